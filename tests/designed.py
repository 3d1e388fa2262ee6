"""Designed-cut corpus (test infrastructure): blocks whose chunk boundaries are chosen, not found.

HDRF's rule (DN/DataDeduplicator.java:264-307): after a cut at p the next cut is after the first
j >= p + 701 with s[j] >= M(p), M(p) = max(0, max s[p .. p + 700]) over signed bytes (no 0 floor for
the block's first chunk), or after p + 1,000,000 when there is none.  So with

  * filler bytes that are all signed-negative (prng_bytes | 0x80),
  * one byte M in [0, 127] inside the window (at p + wpos), and
  * one byte cut >= M at p + L - 1,

the chunk at p is exactly L bytes for any 702 <= L <= 1,000,000; without the cut byte it is the
forced 1,000,001.  The families below place chunk lengths, start alignments, window positions and
thresholds where sha.hip, sha_core.hpp and chunk.hip branch.  Every builder returns
the block together with the END offsets the reference reports for it: the reference drops its last
detected cut and appends the block size, so a block's last chunk is its last designed chunk plus
the tail.

Blocks are generated, cached per process and read-only; nothing here is stored in the tree."""
import functools

import numpy as np

from helpers import prng_bytes

W = 700                       # window: the maximum is taken over s[p .. p + W]
MIN_L = W + 2                 # shortest chunk: the first byte that can cut is s[p + W + 1]
MAX_L = 1_000_000
FORCED = MAX_L + 1            # the forced cut's chunk length
SHA_LONG = 65536              # sha.hip kShaLong: chunks this long go to the long lanes
EDGE_WPOS = (0, 1, 15, 16, 684, 685, 699, 700)
# chunk lengths around the long-lane threshold, SHA padding classes just above it, and the forced cut
LONG_LIST = (65535, 65536, 65537, 65536 + 55, 65536 + 56, 65536 + 63, 65536 + 64, 999_999, 1_000_000)
SEG_LENS = (2808, 14040)      # lane-walk segment lengths at segment_bytes = 1 << 16 and at the default


def _u64(seed, n):
    return prng_bytes(seed, 8 * n).view(np.uint64)


def C(L, M=64, wpos=350, cut=0x7F, decoy=0):
    """One designed chunk: (L, M, wpos, cut, decoy)."""
    return (int(L), int(M), int(wpos), None if cut is None else int(cut), int(decoy))


def _rand_chunk(r, L, decoy=0):
    """Chunk of length L with threshold, window position and cut byte drawn from the word r."""
    r = int(r)
    M = r % 127                                   # < 127: a 0x7F cut byte never ties by accident
    cut = M + (r >> 8) % (128 - M)
    return C(L, M, (r >> 16) % (W + 1), cut, decoy)


def _frozen(a):
    a.flags.writeable = False
    return a


def designed_block(chunks, seed, tail=0, prefix=None):
    """-> (block, end offsets).  chunks: (L, M, wpos, cut, decoy) each; cut None (L == FORCED only)
    leaves the cut byte out; decoy k > 0 writes M - 1 (just under the threshold: must not cut) at
    every k-th byte of the search range from its first byte on, and at its last byte.  prefix:
    (bytes, their end offsets) of a block start that ends with a cut; the chunks follow it."""
    assert 0 <= tail < FORCED
    p = 0 if prefix is None else len(prefix[0])
    total = p + sum(c[0] for c in chunks) + tail
    buf = prng_bytes(seed, total) | np.uint8(0x80)
    ends = []
    if prefix is not None:
        buf[:p] = prefix[0]
        ends = [int(x) for x in prefix[1]]
        assert ends[-1] == p
    for L, M, wpos, cut, decoy in chunks:
        assert MIN_L <= L <= FORCED and 0 <= M <= 127 and 0 <= wpos <= W, (L, M, wpos)
        if decoy:
            buf[p + W + 1:p + L - 1:decoy] = (M - 1) & 0xFF
            if L > MIN_L:
                buf[p + L - 2] = (M - 1) & 0xFF
        buf[p + wpos] = M
        if cut is None:
            assert L == FORCED
        else:
            assert M <= cut <= 127, (M, cut)
            buf[p + L - 1] = cut
        p += L
        ends.append(p)
    return _frozen(buf), np.array(ends[:-1] + [total], np.uint32)


def first_negative_block(m0, L0, seed=1, wpos=350, L1=1500):
    """The first window's maximum is the negative m0, every other byte up to the cut is < m0 and the
    cut byte == m0 (the first chunk's threshold has no 0 floor).  The second chunk's window is all
    negative too, but its threshold is the floor 0: it ignores -1 bytes (which are >= m0) and cuts on
    a 0x00.  A third ordinary chunk and a tail follow.  m0 == -128 leaves no smaller filler: every
    byte of the first chunk is 0x80 and L0 can only be 702."""
    assert -128 <= m0 <= -1 and MIN_L <= L0 <= MAX_L and L1 > MIN_L + 300
    span = m0 + 128                               # filler values -128 .. m0 - 1
    assert span > 0 or L0 == MIN_L
    total = L0 + L1 + MIN_L + 300
    buf = np.uint8(0x80) + prng_bytes(seed, total) % np.uint8(max(span, 1))
    buf[wpos] = m0 & 0xFF
    buf[L0 - 1] = m0 & 0xFF
    p = L0
    buf[[p + 10, p + W + 1, p + W + 300]] = 0xFF  # -1 in the window, at the first search byte, later
    buf[p + L1 - 1] = 0x00                        # ties the floor
    p += L1
    buf[p + 3] = 5
    buf[p + MIN_L - 1] = 0x7F
    return _frozen(buf), np.array([L0, L0 + L1, total], np.uint32)


def interleaved_block(n, spacing=351, value=64, random_from=None, seed=7):
    """Equal markers every `spacing` bytes (351 <= spacing <= 700) over negative filler: a chain cuts
    on every second marker, 2 * spacing-B chunks, so there are two disjoint chains and the block's own
    is the one through markers 2, 4, ...  With random_from the bytes from there on are plain
    prng_bytes, where chains of either parity can meet again; the designed offsets are then unknown
    (None) and the restatements are compared with each other."""
    assert 351 <= spacing <= W and 0 <= value <= 127
    buf = prng_bytes(seed, n) | np.uint8(0x80)
    buf[::spacing] = value
    if random_from is not None:
        buf[random_from:] = prng_bytes(seed + 1, n - random_from)
        return _frozen(buf), None
    ends = [spacing * m + 1 for m in range(2, (n - 1) // spacing + 1, 2)]
    return _frozen(buf), np.array(ends[:-1] + [n], np.uint32)


def interleaved_off_chain(n, spacing, seg_len):
    """(segment starts whose speculative chain runs on the other chain, segment starts after the
    first): a chain started at s cuts first on marker ceil((s + 701) / spacing)."""
    starts = range(seg_len, n, seg_len)
    odd = sum(1 for s in starts if -(-(s + W + 1) // spacing) % 2)
    return odd, len(starts)


# ---- SHA families ------------------------------------------------------------------------------
def _sha_sweep_lengths(seed, n):
    """n lengths in 702..829 whose chunks, laid end to end from offset 0, meet every one of the 512
    classes (len % 128, start % 4): greedy, always towards the start class with most classes left."""
    lo, hi = MIN_L, MIN_L + 128
    need = {(L, a) for L in range(lo, hi) for a in range(4)}
    left = [128] * 4
    out, start = [], 0
    while need:
        a = start % 4
        cands = [L for L in range(lo, hi) if (L, a) in need]
        if cands:
            L = max(cands, key=lambda x: left[(a + x) % 4] - ((a + x) % 4 == a))
            need.discard((L, a))
            left[a] -= 1
        else:
            L = lo + 1                            # 703: an odd step visits every start class
        out.append(L)
        start += L
    assert len(out) <= n
    r = _u64(seed, n)
    out += [lo + int(x) % 128 for x in r[len(out):]]
    return out


@functools.lru_cache(None)
def sha_sweep():
    """(a) ~1,024 chunks of 702..829 B: every (len % 128, start % 4) class."""
    n = 1024
    r = _u64(101, n + 1)
    chunks = [_rand_chunk(r[i], L) for i, L in enumerate(_sha_sweep_lengths(100, n))]
    chunks.append(_rand_chunk(r[n], 777))         # the block's last chunk is not counted
    return designed_block(chunks, 102, tail=41)


@functools.lru_cache(None)
def uneven():
    """(b) ~600 lengths log-uniform in [702, 65535], then 64 equal short chunks, one 60 KB chunk and
    63 short ones: lanes of one wave finish far apart and refill from the pools one by one."""
    n = 600
    r = _u64(201, 2 * n + 200)
    u = r[:n].astype(np.float64) / 2.0 ** 64
    lens = np.minimum(np.floor(MIN_L * (65535.0 / MIN_L) ** u).astype(np.int64), 65535)
    chunks = [_rand_chunk(r[n + i], L) for i, L in enumerate(lens)]
    k = 2 * n
    chunks += [_rand_chunk(r[k + i], 731) for i in range(64)]
    chunks += [_rand_chunk(r[k + 64], 60_000)]
    chunks += [_rand_chunk(r[k + 65 + i], 702 + 3 * i) for i in range(63)]
    chunks += [_rand_chunk(r[k + 128], 800)]
    return designed_block(chunks, 202, tail=13)


def _short(r, i):
    return _rand_chunk(r[i], MIN_L + int(r[i] >> 40) % 300)


def _long(r, i):
    return _rand_chunk(r[i], SHA_LONG + int(r[i] >> 40) % 3000)


@functools.lru_cache(None)
def long_primer():
    """A block that shows the context >= 64 KiB chunks, so the long lanes run for the next batch."""
    r = _u64(301, 16)
    chunks = [_short(r, 0), _long(r, 1), _short(r, 2), _short(r, 3), _long(r, 4), _long(r, 5), _short(r, 6)]
    return designed_block(chunks, 302, tail=5)


@functools.lru_cache(None)
def long_threshold():
    """LONG_LIST and 1,000,001 twice (a natural cut byte at p + 1,000,000, then none), each followed
    by a 702-B chunk."""
    r = _u64(311, 32)
    chunks = []
    for i, L in enumerate(LONG_LIST):
        chunks += [_rand_chunk(r[2 * i], L), _rand_chunk(r[2 * i + 1], MIN_L)]
    chunks += [C(FORCED, 9, 700, 0x7F), C(MIN_L, 3, 0, 3), C(FORCED, 127, 0, None), C(MIN_L, 0, 699, 0)]
    chunks.append(_rand_chunk(r[30], 900))
    return designed_block(chunks, 312, tail=29)


@functools.lru_cache(None)
def long_patterns():
    """(c) the skip path of the ordinary lanes, S short and G >= 64 KiB: a whole reservation of 64 G
    behind 10 S; S and G alternating; G at slot 63 and at slot 0 of a 64-chunk reservation; G in the
    second 1,024-chunk scan tile of the long lanes.  -> [(name, block, offsets)]."""
    out = []
    r = _u64(321, 1400)

    def block(name, kinds, seed):
        chunks = [(_long if g else _short)(r, i) for i, g in enumerate(kinds)]
        chunks.append(_short(r, len(kinds)))      # (merged with the tail: never a G)
        out.append((name,) + designed_block(chunks, seed, tail=17))

    block("10S+64G", [0] * 10 + [1] * 64, 322)
    block("32x(S,G)", [0, 1] * 32, 323)
    block("63S,G,64S,G,S", [0] * 63 + [1] + [0] * 64 + [1] + [0], 324)   # G at chunk 63 and at chunk 128
    block("1100S+G", [0] * 1100 + [1, 0, 1, 1, 0], 325)
    return out


@functools.lru_cache(None)
def drain_batch():
    """(d) 8 blocks of 40 chunks of 65,536 + k B and a few short ones: the long lanes' workgroup 0
    lists 40 per block and drains at >= 256 with entries of several blocks, the rest at the end."""
    out = []
    for b in range(8):
        r = _u64(400 + b, 64)
        chunks = [_short(r, 0), _short(r, 1)]
        chunks += [_rand_chunk(r[2 + i], SHA_LONG + 40 * b + i) for i in range(40)]
        chunks += [_short(r, 50), _short(r, 51)]
        out.append(designed_block(chunks, 420 + b, tail=b))
    return out


BATCH64_SHORT = 4500          # > 32 waves x 2 pools x 64 chunks: what a block's waves reserve up front


@functools.lru_cache(None)
def batch64():
    """A batch of 64 blocks, the most launch_sha takes: each block then has 32 SHA waves, which
    reserve 4,096 chunks before their loops start.  Block 0 holds BATCH64_SHORT short chunks, so its
    last ones come from reservations made inside the loop (after pool Q rotated into P), two G among
    them; blocks 1..62 are two short chunks each; block 63, the highest block number the long lanes
    pack beside a chunk number, holds two G."""
    r = _u64(451, BATCH64_SHORT + 8)
    chunks = [_rand_chunk(r[i], MIN_L + int(r[i] >> 40) % 40) for i in range(BATCH64_SHORT)]
    for i in (4200, 4300):
        chunks[i] = _long(r, i)
    out = [designed_block(chunks, 452, tail=9)]
    for b in range(1, 63):
        rb = _u64(460 + b, 2)
        out.append(designed_block([_short(rb, 0), _short(rb, 1)], 530 + b, tail=b))
    rb = _u64(459, 5)
    out.append(designed_block([_short(rb, 0), _long(rb, 1), _short(rb, 2), _long(rb, 3), _short(rb, 4)], 599, tail=1))
    return out


# ---- chunker families --------------------------------------------------------------------------
def _euler_circuit(n):
    """Every ordered pair (a, c) of 0..n-1 once, as a closed walk from 0 (Hierholzer)."""
    nxt = [0] * n
    stack, walk = [0], []
    while stack:
        a = stack[-1]
        if nxt[a] < n:
            nxt[a] += 1
            stack.append((a + nxt[a]) % n)
        else:
            walk.append(stack.pop())
    walk.reverse()
    assert len(walk) == n * n + 1
    return walk


def _chunk_sweep_chunks():
    """(f) phase / edge-granule sweep, 512 chunks: every pair (start % 16, cut byte % 16) and every
    window position of EDGE_WPOS (the two exact edge granules of the window) at every start % 16,
    twice: 702..717-B chunks, then the same walk with 0..5 more granules of search."""
    walk = _euler_circuit(16)
    r = _u64(501, 520)
    chunks, seen = [], [0] * 16
    for lap in range(2):
        for i in range(256):
            a, c = walk[i], walk[i + 1]           # start class a, next start class c
            k = lap * 256 + i
            L = MIN_L + (c - a - MIN_L) % 16 + 16 * lap * (int(r[k] >> 50) % 6)
            ch = _rand_chunk(r[k], L, decoy=5 if k % 3 == 0 else 0)
            chunks.append(C(L, ch[1], EDGE_WPOS[seen[a] % 8], ch[3], ch[4]))
            seen[a] += 1
    return chunks


@functools.lru_cache(None)
def chunk_sweep():
    return designed_block(_chunk_sweep_chunks() + [C(750, 33, 5, 90)], 502, tail=3)


def _threshold_sweep_chunks():
    """(f) every threshold M in 0..127, once cut by a byte == M (the tie) and once by 0x7F, with
    M - 1 decoys through the search range."""
    r = _u64(511, 260)
    chunks = []
    for M in range(128):
        for j, cut in enumerate((M, 0x7F)):
            x = int(r[2 * M + j])
            chunks.append(C(MIN_L + x % 800, M, (x >> 16) % (W + 1), cut, 1 + (x >> 32) % 9))
    return chunks


@functools.lru_cache(None)
def threshold_sweep():
    return designed_block(_threshold_sweep_chunks() + [C(702, 7, 700, 7)], 512, tail=0)


FIRST_NEGATIVE = ((-128, 702), (-100, 702), (-100, 5000), (-1, 70000))


@functools.lru_cache(None)
def first_negative_blocks():
    return [first_negative_block(m0, L0, seed=520 + i) for i, (m0, L0) in enumerate(FIRST_NEGATIVE)]


def _long_search_chunks(p):
    """(f) searches of 4 KB to 16 KB: L in 4095..4097, then 16,384 + k for k = 0..15, each from a start
    at a multiple of 16 (the short chunk in between realigns), so the match falls on every byte of a
    granule."""
    r = _u64(531, 64)
    chunks = []
    for i, L in enumerate([4095, 4096, 4097] + [16384 + k for k in range(16)]):
        chunks.append(_rand_chunk(r[2 * i], L, decoy=16 if i % 2 else 0))
        p += L
        pad = MIN_L + (-(p + MIN_L)) % 16
        chunks.append(_rand_chunk(r[2 * i + 1], pad))
        p += pad
    return chunks


@functools.lru_cache(None)
def long_search():
    return designed_block(_long_search_chunks(0), 532, tail=11)


UNMET_M0 = -60                # the first window's (unfloored) maximum in unmet_prefix
UNMET_LAST = 6269             # its last marker: the prefix is 351 * 6269 + 1 = 2,200,420 B


def unmet_prefix():
    """A block start after which no speculative chain meets the block's own for 2.2 MB, at either
    segment length (both are multiples of 351).  The first chunk is 1,053 B, cut by a byte equal to
    its negative, unfloored window maximum; equal markers follow at every multiple of 351 from 1,404
    on.  The block's chain, started at 1,053, cuts on the odd markers (5, 7, ...); a chain started
    at a segment start 351 * 8 k or 351 * 40 k cuts on the even ones.  The repair walk of the first
    boundary gives up (kRepairBytes = 2 MiB), so the sequential walk finishes the block: everything
    behind this prefix is cut by walk_chain, not by the lane walk.  -> (bytes, end offsets)."""
    n = 351 * UNMET_LAST + 1
    r = prng_bytes(640, n)
    buf = r | np.uint8(0x80)
    buf[:1053] = np.uint8(0x80) + r[:1053] % np.uint8(UNMET_M0 + 128)
    buf[200] = buf[1052] = UNMET_M0 & 0xFF
    buf[1404::351] = 64
    return buf, [1053] + [351 * m + 1 for m in range(5, UNMET_LAST + 1, 2)]


@functools.lru_cache(None)
def fallback_sweeps():
    """(f) the phase / edge-granule sweep, the threshold sweep and the 4-16 KB searches behind
    unmet_prefix: the same chunks through the sequential walker's general path."""
    pre = unmet_prefix()
    chunks = _chunk_sweep_chunks() + _threshold_sweep_chunks()
    p = len(pre[0]) + sum(c[0] for c in chunks)
    pad = MIN_L + (-(p + MIN_L)) % 16             # the searches start at multiples of 16
    chunks += [C(pad, 2, 1, 2)] + _long_search_chunks(p + pad) + [C(720, 1, 350, 1)]
    return designed_block(chunks, 642, tail=19, prefix=pre)


def _fill_to(chunks, p, end, r, k):
    """Short chunks from p, the last one ending exactly at `end`; -> (p, k)."""
    assert end - p >= MIN_L
    while end - p >= 3004:
        L = MIN_L + int(r[k] >> 40) % 800
        chunks.append(_rand_chunk(r[k], L))
        p, k = p + L, k + 1
    gap = end - p
    for L in ([gap // 2, gap - gap // 2] if gap >= 2 * MIN_L else [gap]):
        chunks.append(_rand_chunk(r[k], L))
        p, k = p + L, k + 1
    return p, k


@functools.lru_cache(None)
def seams(U):
    """(f) cuts at exactly k U - 1, k U and k U + 1; a chunk that starts on a seam with its window
    maximum at wpos 0; one chunk spanning three whole units.  U = 65,536 (a granule-maxima workgroup's
    span) and the lane walk's two segment lengths."""
    r = _u64(541 + U, 1200)
    chunks, p, k = [], 0, 0
    p, k = _fill_to(chunks, p, U - 1, r, k)
    p, k = _fill_to(chunks, p, 2 * U, r, k)
    chunks.append(C(MIN_L + 33, 17, 0, 17))                        # starts on the seam, maximum at wpos 0
    p += MIN_L + 33
    p, k = _fill_to(chunks, p, 3 * U + 1, r, k)
    chunks.append(_rand_chunk(r[k], 7 * U + 5 - p))                # units 4, 5 and 6 whole in one chunk
    p, k = 7 * U + 5, k + 1
    p, k = _fill_to(chunks, p, 9 * U, r, k)
    chunks.append(C(2 * U, 0, 0, 0))                               # seam to seam, M == cut == 0
    chunks.append(_rand_chunk(r[k], 740))
    return designed_block(chunks, 542, tail=7)


@functools.lru_cache(None)
def interleaved(spacing, random_from):
    return interleaved_block(1 << 20, spacing=spacing, random_from=random_from)


END_CLASSES = (0, 1, 55, 56, 63)


@functools.lru_cache(None)
def end_blocks():
    """(g) 16 small blocks whose last chunks (last designed chunk + tail) take len % 64 from
    END_CLASSES[i % 5] and start % 4 == i % 4."""
    out = []
    for i in range(16):
        r = _u64(600 + i, 8)
        lens = [MIN_L + int(r[j] >> 40) % 900 for j in range(3)]
        lens[2] += (i % 4 - sum(lens)) % 4
        tail = 5 + i
        last = MIN_L + 3 * i
        last += (END_CLASSES[i % 5] - last - tail) % 64
        chunks = [_rand_chunk(r[j], L) for j, L in enumerate(lens + [last])]
        out.append(designed_block(chunks, 620 + i, tail=tail))
    return out


# ---- bookkeeping families: the lane walk's overrun, the repair, the stitch (tests/lane_model.py) ---
# Blocks whose only non-negative bytes are placed markers.  With equal markers the rule reduces to
# "the next cut is one past the first marker at or beyond p + 701", so a lattice of markers every d
# bytes (351 <= d <= 700) carries two disjoint chains, on the even and on the odd markers, and both
# segment lengths are multiples of d: every segment's speculative chain starts on the even one.
# Deleting one marker moves the chain that would have cut on it to the next marker, i.e. onto the
# other chain; a chain already there is not touched.  So:
#   * deleting the even marker at a segment start S (a + 1) sends segment a's chain onto the odd
#     markers in its overrun, where the next segment's (even) chain never meets it: the boundary fails
#     at the overrun cut seg_len or more past the segment end, or at its kLaneOver-th overrun cut;
#   * deleting an odd marker further on brings it back, onto a cut of the segment that holds it: at
#     overrun cut i (a sync at (i, i)) or at the repair's cut r (a jump with n_ext = r).
def marker_ends(n, marks):
    """End offsets under the rule stated on markers alone ({position: value}; every other byte is
    negative and the first window holds a marker)."""
    import bisect
    pos = sorted(marks)
    val = [marks[p] for p in pos]
    ends, p = [], 0
    while p + W <= n - 1:
        a, b = bisect.bisect_left(pos, p), bisect.bisect_left(pos, p + W + 1)
        assert p > 0 or b > a, "the first window needs a marker"
        m = max([0] + val[a:b])
        i = b
        while i < len(pos) and val[i] < m:
            i += 1
        if i < len(pos) and pos[i] <= min(p + MAX_L, n - 1):
            p = pos[i] + 1
        elif p + MAX_L <= n - 1:
            p += FORCED
        else:
            break
        ends.append(p)
    return np.array(ends[:-1] + [n], np.uint32)


def marker_block(n, marks, seed):
    buf = prng_bytes(seed, n) | np.uint8(0x80)
    pos = np.fromiter(marks.keys(), np.int64, len(marks))
    buf[pos] = np.fromiter(marks.values(), np.uint8, len(marks))
    return _frozen(buf), marker_ends(n, marks)


def lattice_fail_cuts(seg_len, d, lane_over=8):
    """overrun cuts a chain on the odd markers records before its boundary fails"""
    return min(seg_len // d // 2, lane_over - 1) + 1


def lattice_episodes(seg_len, d, script, seed, a0=1, tail_segs=2, tail_bytes=1234, lane_over=8):
    """A lattice block (spacing d) with one scripted event after another on the block's own chain.
    The chain is on the even markers in segment a; events:
      ("sync", i)         segment a's chain leaves for the odd markers at its end and is back at overrun
                          cut i, which is the next segment's cut i: sync (i, i); a += 1
      ("repair", r)       it leaves and is back at the repair's cut r, a main cut of the segment m
                          holding it: jump, n_ext = r (r + 1 when cut r is one past a segment start,
                          an overrun cut of segment m - 1: not matched); a = m
      ("repair", r, off)  also segments a + b, b in off, leave at their ends: failed boundaries that the
                          jump passes over
      ("at", k)           the next event is at segment k (>= a)
      ("leave",)          it leaves and never returns (the last event)
    -> (block, end offsets, [(event, segment, target segment or None)])."""
    S = seg_len // d
    assert S * d == seg_len and S % 2 == 0 and 351 <= d <= W
    nf = lattice_fail_cuts(seg_len, d, lane_over)
    deleted, log, a = set(), [], a0
    for ev in script:
        if ev[0] == "at":
            assert ev[1] >= a
            a = ev[1]
        elif ev[0] == "sync":
            deleted |= {S * (a + 1), S * (a + 1) + 2 * ev[1] + 1}
            log.append((ev, a, a + 1))
            a += 1
        elif ev[0] == "repair":
            first_odd = S * (a + 1) + 2 * nf - 1          # the failing overrun cut's marker
            back = first_odd + 2 * ev[1] + 1
            deleted |= {S * (a + 1), back - 1}
            for b in (ev[2] if len(ev) > 2 else ()):
                assert S * (a + b + 1) < back - 2
                deleted.add(S * (a + b + 1))
            m = (back + (2 if back % S == 0 else 0)) // S
            log.append((ev, a, m))
            a = m
        else:
            assert ev[0] == "leave" and ev is script[-1]
            deleted.add(S * (a + 1))
            log.append((ev, a, None))
    n = (a + tail_segs) * seg_len + tail_bytes
    marks = {d * j: 64 for j in range((n - 1) // d + 1) if j not in deleted}
    return marker_block(n, marks, seed) + (log,)


# n_ext values the issue names (the kept-cuts path's 64 / 65 and the list sink's 64 / 128 edges), and
# more for jmp in {1, 2, 3, >= 8} and jj in {0, 1, last main cut}; per (seg_len, d): the lattice gives
# a cut r a main-cut landing unless (first landing + 2 r) % S == 0
REPAIR_N_EXT = (2, 3, 63, 64, 65, 66, 128, 129, 130)
REPAIR_SCRIPTS = {
    (2808, 351): (1, 2, 4, 64, 65, 66, 128, 129, 130),    # r % 4 == 3 lands one past a segment start
    (2808, 468): (3, 63),
    (14040, 351): (1, 2, 3, 11, 13, 14, 20, 40, 63, 64, 65, 66, 128, 129, 130, 160),
}


@functools.lru_cache(None)
def repair_sweep(seg_len, d, hole=False):
    """(B) on-path repairs with the n_ext of REPAIR_SCRIPTS, back to back, the first at segment 62 (the
    first wave's last lane, which reads the helper lane's list; hole: at segment 63, the next wave's
    lane 0); the repairs of n_ext >= 64 pass over two failed boundaries, the first next to the on-path
    one.  hole: every repair comes back one past a segment start instead, an overrun cut of the
    segment before (met, not matched) and is matched one cut on."""
    rs = REPAIR_SCRIPTS[(seg_len, d)]
    S = seg_len // d
    script = [("at", 63 if hole else 62)]
    for r in rs:
        if hole:
            r = next(x for x in range(r, r + S) if (2 * lattice_fail_cuts(seg_len, d) + 2 * x) % S == 0)
        script.append(("repair", r, (1, 2)) if r >= 64 else ("repair", r))
    return lattice_episodes(seg_len, d, script, 700 + d + (1 if hole else 0))


@functools.lru_cache(None)
def overrun_sweep(seg_len):
    """(A) syncs at overrun cut number 1, 2, ... (every one the segment length leaves room for, up to
    kLaneOver = 8), at lanes 62 and 63 of the first wave among others; then a chain that leaves for
    good two segments before the block end."""
    idx = [i for i in (0, 1, 2, 6, 7) if 2 * i + 2 < seg_len // 351]    # the shared cut lies inside the next segment
    script = [("sync", i) for i in idx] + [("at", 62), ("sync", 0), ("sync", 1), ("at", 70)] + \
             [("sync", i) for i in idx] + [("leave",)]
    return lattice_episodes(seg_len, 351, script, 720 + seg_len % 97, tail_segs=2, tail_bytes=900)


@functools.lru_cache(None)
def small_blocks(seg_len):
    """(A) blocks of exactly 1 and 2 segments, and 2 segments plus one byte."""
    out = []
    for i, n in enumerate((seg_len, 2 * seg_len, 2 * seg_len + 1)):
        marks = {351 * j: 64 for j in range((n - 1) // 351 + 1) if j != seg_len // 351}
        out.append(marker_block(n, marks, 730 + i))
    return out


def _background(lo, hi, step=936, phase=467):
    """markers of one chain (spacing >= 702) at step * j + phase within [lo, hi)"""
    j0 = -(-(lo - phase) // step)
    return {step * j + phase: 64 for j in range(max(j0, 0), (hi - phase + step - 1) // step) if step * j + phase < hi}


def _edge_start(seg_len, a_min, back, capped):
    """-> (a, P): a segment a >= a_min and a cut P in it, more than 701 B before its end, from which the
    search for the byte target - 1, target = (a + 2) * seg_len - back, reads a last 1-KiB view (views
    start at P & ~63) that begins within 16 B beyond over_lim = (a + 2) * seg_len - 64 (capped: the search
    is given up) / within 16 B at or before it (it is not)."""
    for a in range(a_min, a_min + 8):
        over_lim, target = (a + 2) * seg_len - 64, (a + 2) * seg_len - back
        for P in range((a + 1) * seg_len - 720, a * seg_len + 800, -1):
            b0 = P & ~63
            vs = b0 + 1024 * ((target - 1 - b0) // 1024)
            if (0 < vs - over_lim <= 16) if capped else (0 <= over_lim - vs < 16):
                return a, P
    raise AssertionError("no such start")


EDGE_KINDS = ("last_byte", "last_byte_capped", "one_past", "at_over_lim", "below_over_lim")


@functools.lru_cache(None)
def overrun_edges(seg_len):
    """(A) one chain (markers >= 702 B apart), and at five boundaries a (e = the next segment's start)
    one long chunk from a cut P in segment a:
      last_byte         to the cut e + seg_len - 1, the next segment's first cut: sync (0, 0); the search's
                        last view begins less than 16 B before over_lim
      last_byte_capped  the same cut from a P whose search would read a view that begins at most 16 B
                        beyond over_lim: fails
                        with no overrun cut, and the repair's first cut is shared (n_ext 1, jmp 1)
      one_past          to the cut e + seg_len exactly: fails, although it is the next segment's cut
      at_over_lim       a cut at over_lim that the next segment's chain passes over (a 100-valued
                        marker inside the window of its 64-valued cut): fails there, one overrun cut
      below_over_lim    the same one byte earlier: goes on, and fails at its next cut (two)
    -> (block, end offsets, {kind: segment a})."""
    marks, where = {}, {}
    a, lo = 3, 0
    for kind in EDGE_KINDS:
        if kind in ("last_byte", "last_byte_capped", "one_past"):
            a, P = _edge_start(seg_len, a, 0 if kind == "one_past" else 1, kind == "last_byte_capped")
            c = (a + 2) * seg_len - (0 if kind == "one_past" else 1)
            marks.update(_background(lo, P - 702))
            marks[P - 1] = 64
            marks[c - 1] = 64
            lo = c - 1 + 702
        else:
            e = (a + 1) * seg_len
            c = e + seg_len - 64 - (1 if kind == "below_over_lim" else 0)
            P = e - 300
            marks.update(_background(lo, P - 702))
            marks[P - 1] = 64
            marks[P + 5] = 100                       # P's window: its chain passes every 64
            marks[c - 300 - 1] = 64                  # the next segment's first cut; its window holds c - 1
            marks[c - 1] = 100
            marks[c + 800] = 100                     # the next cut of both
            lo = c + 800 + 702
        where[kind] = a
        a = lo // seg_len + 4
    n = (a + 2) * seg_len + 555
    marks.update(_background(lo, n))
    marks.setdefault(100, 64)                        # the first window's marker
    return marker_block(n, marks, 740 + seg_len % 97) + (where,)


REPAIR_P0 = 1500              # repair_bytes_blocks: the failed chain's last cut, at either segment length


@functools.lru_cache(None)
def repair_bytes_blocks():
    """(B) segment 0's chain cuts at 702 and 1,500 and then runs three long chunks, the first two
    ending within the first 701 B of a segment (of either length: no list holds those cuts), the third
    at REPAIR_P0 + kRepairBytes exactly, a main cut of its segment: the repair merges there.  In the
    second block that cut is one byte later: the repair gives up and the sequential walk finishes the
    block from the two cuts the stitch produced.  -> [(block, end offsets)] (exact, one past)."""
    out = []
    for extra in (0, 1):
        c1, c2 = 14040 * 71 + 300, 14040 * 142 + 300
        c3 = REPAIR_P0 + (2 << 20) + extra
        assert min(c3 % 2808, c3 % 14040) >= 702 + 2 and max(c1 - REPAIR_P0, c2 - c1) <= MAX_L
        chunks = [C(702, 5, 10, 5), C(REPAIR_P0 - 702, 7, 3, 7), C(c1 - REPAIR_P0, 100, 8, 110), C(c2 - c1, 100, 8, 110),
                  C(c3 - c2, 100, 8, 110), C(900, 9, 600, 9), C(5000, 9, 2, 40), C(750, 1, 1, 1)]
        out.append(designed_block(chunks, 750 + extra, tail=77))
    return out


RQ_KEEP = 16384               # common.hpp kRqKeep
QUEUE_SURPLUS = 4096


@functools.lru_cache(None)
def queue_batch(blocks=8, surplus=QUEUE_SURPLUS):
    """(C) one batch at seg_len 2,808 whose failed boundaries number >= kRqKeep + surplus: repairs back
    to back, every second segment a failed boundary on the block's path, each merging within 2 cuts
    (n_ext 2, every third 1) except every 97th (n_ext 64, 65, 66, 129 in turn): which of them get queue positions
    at or above kRqKeep is up to the atomics."""
    per = -(-(RQ_KEEP + surplus) // blocks)
    out = []
    for b in range(blocks):
        long_r = (64, 65, 66, 129)
        script = []
        for i in range(per):
            script.append(("repair", long_r[(i // 97) % 4] if i % 97 == 96 else (2 if (i + b) % 3 else 1)))
        out.append(lattice_episodes(2808, 351, script, 760 + b, a0=1 + b % 3, tail_bytes=100 + 17 * b)[:2])
    return out


STITCH_NODES = 1024           # chunk.hip kStitchNodes


@functools.lru_cache(None)
def stitch_windows(seg_len, give_up):
    """(D) more than 2 x kStitchNodes irregular boundaries in one block: repairs back to back (every
    jump's target is the next irregular boundary, so the jump from the last node of a window lands on
    the first node of the next), eight of them passing over two failed boundaries each; the path ends
    inside the third window: the chain leaves for good and runs to the block end within its overrun
    (END), or (give_up) fails and its repair runs out of data, so the sequential walk starts from the
    offsets all three windows produced."""
    rs = REPAIR_SCRIPTS[(seg_len, 351)]
    short = [r for r in rs if r < 12]
    script = []
    for i in range(2 * STITCH_NODES + 40):
        script.append(("repair", 64 + i % 3, (1, 2)) if i % 256 == 200 else ("repair", short[i % len(short)]))
    script.append(("leave",))
    tail = (6, 77) if give_up else (1, 1500)
    return lattice_episodes(seg_len, 351, script, 780 + seg_len % 97 + give_up, tail_segs=tail[0], tail_bytes=tail[1])
