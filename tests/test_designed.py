"""Designed-cut corpus (tests/designed.py): chunking and SHA pinned at chosen chunk boundaries.

The data-driven tests reach sha.hip and chunk.hip only through cuts that fall where they happen to
(702..3000-B chunks, or forced 1,000,001-B ones).  Here every chunk length, start alignment, window
position and threshold is placed: the SHA lanes' refill and pool rotation, the long-lane threshold
(kShaLong), its mid-scan drain and the ordinary lanes' skip path, sha_chunk (HDRF_SHA_CARRY=0), the
chunker's general path (no 0x7F byte in any window: the filler is signed-negative), its edge granules,
long searches, seams, chains that never meet, and the first chunk's unfloored threshold.

CPU tests: the C oracle and the two Python restatements return exactly the designed offsets, hashlib
agrees with the oracle's digests, and the coverage each family claims is asserted as complete sets
(over chunks that are not their block's last).  GPU tests: every block against Oracle.reduce through
compare_block / compare_state, bit-exact, and the stored result read back (scrub, verified rebuild,
ranged reads across designed cuts)."""
import collections
import hashlib
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import designed as D
from helpers import compare_block, compare_state
from hdrf_amd.lib import Context
from oracle import pyref
from oracle.oracle import Oracle, chunk as ora_chunk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

IL_SPACINGS = (351, 353)      # 351: the two chains; 353: segment starts of either length land on both


def _family(name):
    """-> [(tag, block, designed offsets or None)]"""
    if name == "long_patterns":
        return D.long_patterns()
    if name == "first_negative":
        return [(f"m0={m0} L0={L0}",) + b for (m0, L0), b in zip(D.FIRST_NEGATIVE, D.first_negative_blocks())]
    if name == "seams":
        return [(f"U={U}",) + D.seams(U) for U in (65536,) + D.SEG_LENS]
    if name == "interleaved":
        return [(f"spacing={s} random_from={rf}",) + D.interleaved(s, rf) for s in IL_SPACINGS for rf in (None, 1 << 19)]
    if name == "end_blocks":
        return [(f"end {i}",) + b for i, b in enumerate(D.end_blocks())]
    return [(name,) + getattr(D, name)()]


FAMILIES = ["sha_sweep", "uneven", "long_primer", "long_threshold", "long_patterns", "chunk_sweep", "threshold_sweep",
            "first_negative", "long_search", "fallback_sweeps", "seams", "interleaved", "end_blocks"]


def _chunks(offs, start_from=0):
    """(starts, lengths) of the chunks that are not the block's last (and start at start_from or later)."""
    offs = np.asarray(offs, np.int64)
    starts = np.concatenate([[0], offs[:-1]])
    keep = starts[:-1] >= start_from
    return starts[:-1][keep], (offs - starts)[:-1][keep]


def _signed(blk):
    return blk.view(np.int8)


# ---- CPU: the designed offsets are the reference's ----------------------------------------------
@pytest.mark.parametrize("name", FAMILIES)
def test_cuts_three_restatements(name):
    for tag, blk, offs in _family(name):
        raw = blk.tobytes()
        o = list(ora_chunk(blk))
        if offs is not None:
            assert o == list(offs), f"{name} {tag}: the C oracle's cuts are not the designed ones"
        assert pyref.chunking(raw) == o, f"{name} {tag}: pyref.chunking"
        assert pyref.chunking_closed_form(raw) == o, f"{name} {tag}: pyref.chunking_closed_form"


def test_cuts_drain_batch_oracle():
    for i, (blk, offs) in enumerate(D.drain_batch()):
        assert np.array_equal(ora_chunk(blk), offs), f"drain block {i}"
        starts, lens = _chunks(offs)
        assert np.count_nonzero(lens >= D.SHA_LONG) == 40 and len(offs) <= 1024    # one scan tile each


def test_cuts_batch64_oracle():
    blocks = D.batch64()
    assert len(blocks) == 64
    for i, (blk, offs) in enumerate(blocks):
        assert np.array_equal(ora_chunk(blk), offs), f"batch64 block {i}"
    g = np.nonzero(_chunks(blocks[0][1])[1] >= D.SHA_LONG)[0]
    assert g.tolist() == [4200, 4300] and len(blocks[0][1]) > 32 * 2 * 64 + 256     # past the up-front reservations
    assert (_chunks(blocks[63][1])[1] >= D.SHA_LONG).sum() == 2
    assert max(len(b) for b, _ in blocks) <= 4 << 20


@pytest.mark.parametrize("hasher", [0, 1])
def test_digests_hashlib_equals_oracle(hasher):
    blk, offs = D.sha_sweep()
    h = hashlib.sha1 if hasher == 0 else hashlib.sha224
    o = Oracle(hasher=hasher).reduce(blk, 1)
    assert np.array_equal(o["offsets"], offs)
    raw = blk.tobytes()
    starts = [0] + list(offs[:-1])
    for j, (a, b) in enumerate(zip(starts, offs)):
        assert bytes(o["digests"][j]) == h(raw[a:b]).digest(), j


# ---- CPU: coverage, as complete sets ------------------------------------------------------------
def test_coverage_sha_sweep():
    starts, lens = _chunks(D.sha_sweep()[1])
    assert lens.min() >= 702 and lens.max() <= 829 and len(lens) >= 1024
    got = set(zip((lens % 128).tolist(), (starts % 4).tolist()))
    assert got == {(r, a) for r in range(128) for a in range(4)}


@pytest.mark.parametrize("family", ["chunk_sweep", "fallback_sweeps"])
def test_coverage_chunk_sweep(family):
    blk, offs = getattr(D, family)()
    starts, lens = _chunks(offs, 0 if family == "chunk_sweep" else len(D.unmet_prefix()[0]))
    assert len(lens) >= 512
    pairs = set(zip((starts % 16).tolist(), ((starts + lens - 1) % 16).tolist()))
    assert pairs == {(a, b) for a in range(16) for b in range(16)}
    s = _signed(blk)
    wpos = [int(np.argmax(s[p:p + D.W + 1])) for p in starts]       # read back from the bytes
    got = set(zip((starts % 16).tolist(), wpos))
    assert got >= {(a, w) for a in range(16) for w in D.EDGE_WPOS}


@pytest.mark.parametrize("family", ["threshold_sweep", "fallback_sweeps"])
def test_coverage_threshold_sweep(family):
    blk, offs = getattr(D, family)()
    starts, lens = _chunks(offs, 0 if family == "threshold_sweep" else len(D.unmet_prefix()[0]))
    s = _signed(blk)
    got = collections.Counter((int(s[p:p + D.W + 1].max()), int(s[p + n - 1])) for p, n in zip(starts, lens))
    want = collections.Counter()
    for M in range(128):
        want[(M, M)] += 1
        want[(M, 127)] += 1
    if family == "threshold_sweep":
        assert got == want
        for p, n in zip(starts, lens):                               # decoys: M - 1 at the first search byte
            if n > D.MIN_L:
                assert int(s[p + D.W + 1]) == int(s[p:p + D.W + 1].max()) - 1
    else:                                                            # (among the other sweeps' chunks)
        assert not want - got


def test_coverage_long_and_search_lists():
    blk, offs = D.long_threshold()
    starts, lens = _chunks(offs)
    ll = lens.tolist()
    want = list(D.LONG_LIST) + [D.FORCED, D.FORCED]
    assert [n for n in ll if n > 702] == want
    for i, n in enumerate(ll):                                       # each followed by a 702-B chunk
        if n > 702:
            assert ll[i + 1] == 702
    s = _signed(blk)
    f = [int(p) for p, n in zip(starts, lens) if n == D.FORCED]
    m = [max(0, int(s[p:p + D.W + 1].max())) for p in f]
    assert int(s[f[0] + D.MAX_L]) >= m[0], "a natural cut on the forced cut's byte"
    assert int(s[f[1] + D.MAX_L]) < m[1], "no natural cut: the forced one alone"
    for fam in (D.long_search, D.fallback_sweeps):
        starts, lens = _chunks(fam()[1])
        big = lens >= 4095
        assert lens[big].tolist() == [4095, 4096, 4097] + [16384 + k for k in range(16)]
        assert not (starts[big] % 16).any()
        assert set(((starts + lens - 1)[lens >= 16384] % 16).tolist()) == set(range(16))


def test_coverage_unmet_prefix():
    """No speculative chain of the prefix shares a cut with the block's own, at either segment length,
    and the prefix outlasts the repair walk (kRepairBytes past segment 0's last cut)."""
    blk, ends = D.unmet_prefix()
    n = len(blk)
    own = set(ends)
    assert ends[0] == 1053 and int(_signed(blk)[:701].max()) == D.UNMET_M0 and ends[-1] == n
    for seg in D.SEG_LENS:
        assert seg % 351 == 0
        for s in range(seg, n - 2 * D.MIN_L, seg):
            m = -(-(s + D.W + 1) // 351)                              # the chain from s cuts on markers m, m + 2, ...
            assert m % 2 == 0 and 351 * m + 1 not in own
        assert n > 2 * seg + (2 << 20) + 4096


def test_coverage_long_patterns():
    pat = {name: _chunks(offs)[1] >= D.SHA_LONG for name, _, offs in D.long_patterns()}
    g = pat["10S+64G"]
    assert not g[:10].any() and g[10:74].all()                       # a whole reservation (64..127) of G inside
    g = pat["32x(S,G)"]
    assert g.tolist() == [False, True] * 32
    g = pat["63S,G,64S,G,S"]
    assert np.nonzero(g)[0].tolist() == [63, 128]                    # slot 63 and slot 0 of a 64-chunk reservation
    g = pat["1100S+G"]
    assert np.nonzero(g)[0].min() >= 1024 and g.sum() == 3           # the long lanes' second scan tile
    assert (_chunks(D.long_primer()[1])[1] >= D.SHA_LONG).sum() >= 2
    starts, lens = _chunks(D.uneven()[1])
    assert lens.max() < D.SHA_LONG and (lens > 3000).sum() > 300 and (lens < 3000).sum() > 150


def test_coverage_seams_and_interleaved():
    for U in (65536,) + D.SEG_LENS:
        blk, offs = D.seams(U)
        o = set(offs.tolist())
        assert {U - 1, 2 * U, 3 * U + 1, 9 * U, 11 * U} <= o
        starts, lens = _chunks(offs)
        i = starts.tolist().index(2 * U)
        assert int(np.argmax(_signed(blk)[2 * U:2 * U + D.W + 1])) == 0
        assert 3 * U + 1 in starts.tolist() and 7 * U + 5 in o      # units 4..6 inside one chunk
        assert lens[starts.tolist().index(3 * U + 1)] == 4 * U + 4 and i >= 0
    n = 1 << 20
    # 351 = seg_len / 8 and seg_len / 40: every segment start lands on the block's own chain; at
    # multiples of 65,536 8 of 15 starts land on the other one.  353 splits the lane walk's segments.
    assert D.interleaved_off_chain(n, 351, 65536) == (8, 15)
    for seg in D.SEG_LENS:
        assert D.interleaved_off_chain(n, 351, seg)[0] == 0
        odd, tot = D.interleaved_off_chain(n, 353, seg)
        assert tot // 4 < odd < 3 * tot // 4, (seg, odd, tot)


def test_coverage_end_blocks():
    got = set()
    for blk, offs in D.end_blocks():
        start = int(offs[-2])
        got.add(((len(blk) - start) % 64, start % 4))
    assert {c for c, _ in got} == set(D.END_CLASSES) and {a for _, a in got} == {0, 1, 2, 3} and len(got) == 16


# ---- GPU ---------------------------------------------------------------------------------------
CFG = dict(max_block_bytes=16 << 20, max_batch_blocks=8, index_log2=20, arena_slots=64)


def _sample_cuts(offs):
    """A fixed sample of a block's cuts: every n/8-th, the ends of its long chunks, the last two."""
    offs = np.asarray(offs, np.int64)
    n = len(offs)
    lens = offs - np.concatenate([[0], offs[:-1]])
    idx = set(range(0, n, max(1, n // 8))) | set(np.nonzero(lens >= D.SHA_LONG)[0][:24].tolist()) | {n - 1, max(0, n - 2)}
    return [int(offs[i]) for i in sorted(idx)]


def check_stored(ctx, stored):
    """(h) the stored result: a clean scrub of every entry, the verified rebuild, reads across cuts."""
    st, bad = ctx.scrub()
    assert st["bad"] == 0 and not bad, bad[:3]
    assert st["checked"] == ctx.index_count()
    for bid, blk, offs in stored:
        assert np.array_equal(ctx.reconstruct_block(bid, verify=True), blk), f"block {bid:#x} not rebuilt"
        for cut in _sample_cuts(offs):
            lo = max(0, cut - 3)
            assert np.array_equal(ctx.read_range(bid, lo, 6), blk[lo:lo + 6]), f"block {bid:#x} range at cut {cut}"


def reduce_blocks(ctx, ora, blocks, bid0, tag=""):
    """reduce_block of each (block, designed offsets) against the oracle; -> [(bid, block, offsets)]."""
    stored = []
    for i, (blk, offs) in enumerate(blocks):
        bid = bid0 + 7 * i
        g = ctx.reduce_block(blk, bid)
        o = ora.reduce(blk, bid)
        compare_block(g, o, tag=f"{tag} block {i}")
        if offs is not None:
            assert np.array_equal(g["offsets"], offs), f"{tag} block {i}: not the designed cuts"
        stored.append((bid, blk, g["offsets"]))
    return stored


def reduce_device_batch(ctx, ora, blocks, bids, fill=0, exact=False, tag=""):
    """One reduce_batch of blocks placed in device memory at 16-B aligned offsets, the gaps (64..111 B)
    holding `fill`; exact: readable is the contract's minimum, len + 64."""
    offs, o = [], 0
    for blk, _ in blocks:
        offs.append(o)
        o = (o + len(blk) + 64 + 15) // 16 * 16 + 16 * (len(offs) % 3)
    buf = np.full(o + 64, fill, np.uint8)
    for (blk, _), p in zip(blocks, offs):
        buf[p:p + len(blk)] = blk
    dev = ctx.dev_alloc(buf.size)
    ctx.h2d(dev, buf)
    readable = [len(b) + 64 if exact else buf.size - p for (b, _), p in zip(blocks, offs)]
    ctx.reduce_batch([dev + p for p in offs], [len(b) for b, _ in blocks], readable, bids)
    for i, (blk, want) in enumerate(blocks):
        g = ctx.batch_result(i)
        compare_block(g, ora.reduce(blk, bids[i]), tag=f"{tag} batch block {i}")
        assert np.array_equal(g["offsets"], want), f"{tag} batch block {i}: not the designed cuts"
    ctx.dev_free(dev)


def case_sha_sweep(hasher):
    """(a) the 512-class block twice: the second time every chunk is a duplicate."""
    blk, offs = D.sha_sweep()
    ctx = Context(hasher=hasher, **CFG)
    ora = Oracle(hasher=hasher)
    stored = reduce_blocks(ctx, ora, [(blk, offs)], 0x1000, tag="sha sweep")
    g = ctx.reduce_block(blk, 0x2000)
    compare_block(g, ora.reduce(blk, 0x2000), tag="sha sweep again")
    assert not g["is_new"].any() and g["store_size"] == 0
    compare_state(ctx, ora, [0x1000, 0x2000])
    check_stored(ctx, stored + [(0x2000, blk, offs)])
    ctx.close()


def case_long(hasher):
    """(c) the primer shows the context >= 64 KiB chunks (hdrf_wait_batch turns the long lanes on
    for the next submissions); every later block holds some too, so they stay on."""
    blocks = [D.long_primer(), D.long_threshold()] + [(b, o) for _, b, o in D.long_patterns()]
    kw = dict(CFG, max_block_bytes=32 << 20)
    ctx = Context(hasher=hasher, **kw)
    ora = Oracle(hasher=hasher)
    stored = reduce_blocks(ctx, ora, blocks, 0x3000, tag="long")
    compare_state(ctx, ora, [s[0] for s in stored])
    check_stored(ctx, stored)
    ctx.close()


def case_end_blocks():
    """(g) two device batches of 8 blocks, 0x7F in the gaps, readable exactly len + 64."""
    blocks = D.end_blocks()
    ctx = Context(**CFG)
    ora = Oracle()
    ids = []
    for b0 in (0, 8):
        bids = [0x5000 + b0 + i for i in range(8)]
        reduce_device_batch(ctx, ora, blocks[b0:b0 + 8], bids, fill=0x7F, exact=True, tag=f"ends {b0}")
        ids += bids
    compare_state(ctx, ora, ids)
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("hasher", [0, 1])
def test_sha_class_sweep(hasher):
    case_sha_sweep(hasher)


@pytest.mark.gpu
@pytest.mark.parametrize("hasher", [0, 1])
def test_sha_uneven_lanes(hasher):
    """(b) lanes of one wave finish far apart: the refill (ballot / rank / head), the rotation of
    pool P to Q and the carry reset on a new chunk."""
    ctx = Context(hasher=hasher, **CFG)
    ora = Oracle(hasher=hasher)
    stored = reduce_blocks(ctx, ora, [D.uneven()], 0x2100, tag="uneven")
    compare_state(ctx, ora, [s[0] for s in stored])
    check_stored(ctx, stored)
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("hasher", [0, 1])
def test_sha_long_threshold_and_skip_patterns(hasher):
    case_long(hasher)


@pytest.mark.gpu
def test_sha_long_drain_mid_scan_across_blocks():
    """(d) after a primer batch, one batch of 8 blocks x 40 long chunks: the long lanes' workgroup 0
    drains at >= 256 entries holding chunks of several blocks (the block << 26 | chunk packing), and
    the remainder at the end."""
    blocks = D.drain_batch()
    ctx = Context(hasher=1, **CFG)
    ora = Oracle(hasher=1)
    reduce_device_batch(ctx, ora, [D.long_primer()], [0x4000], tag="primer")
    bids = [0x4100 + i for i in range(8)]
    reduce_device_batch(ctx, ora, blocks, bids, tag="drain")
    compare_state(ctx, ora, [0x4000] + bids)
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("hasher", [0, 1])
def test_sha_batch_of_64_blocks_refills_in_loop(hasher):
    """A 64-block batch leaves each block 32 SHA waves: block 0's 4,500 chunks outlast the two pools
    every wave reserves up front, so waves rotate Q into P and reserve again inside the loop, and skip
    long chunks found there; block 63's long chunks carry the highest block number through the long
    lanes' block << 26 | chunk packing.  After a primer batch, so the long lanes run."""
    blocks = D.batch64()
    ctx = Context(hasher=hasher, **dict(CFG, max_block_bytes=4 << 20, max_batch_blocks=64))
    ora = Oracle(hasher=hasher)
    reduce_device_batch(ctx, ora, [D.long_primer()], [0x4800], tag="primer")
    bids = [0x4900 + i for i in range(64)]
    reduce_device_batch(ctx, ora, blocks, bids, tag="batch64")
    compare_state(ctx, ora, [0x4800] + bids)
    ctx.close()


@pytest.mark.gpu
def test_block_ends_at_contract_minimum():
    case_end_blocks()


SEGS = [1 << 16, None]        # lane-walk segments of 2,808 B and the default's 14,040 B


def _chunker_ctx(seg):
    kw = dict(CFG) if seg is None else dict(CFG, segment_bytes=seg)
    return Context(**kw), Oracle()


@pytest.mark.gpu
@pytest.mark.parametrize("seg", SEGS)
@pytest.mark.parametrize("group", ["sweeps", "long", "fallback", "seams", "interleaved"])
def test_chunker_families(group, seg):
    """(f) the chunker's general path at designed cuts."""
    blocks = {"sweeps": lambda: [D.chunk_sweep(), D.threshold_sweep()],
              "long": lambda: [D.long_search(), D.long_threshold()],
              "fallback": lambda: [D.fallback_sweeps()],
              "seams": lambda: [D.seams(U) for U in (65536,) + D.SEG_LENS],
              "interleaved": lambda: [D.interleaved(s, rf) for s in IL_SPACINGS for rf in (None, 1 << 19)]}[group]()
    ctx, ora = _chunker_ctx(seg)
    stored = reduce_blocks(ctx, ora, blocks, 0x6000, tag=group)
    compare_state(ctx, ora, [s[0] for s in stored])
    check_stored(ctx, stored)
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("seg", SEGS)
def test_chunker_first_negative_batch(seg):
    """(f) the first chunk's unfloored threshold, four blocks as one batch."""
    ctx, ora = _chunker_ctx(seg)
    bids = [0x7000 + i for i in range(4)]
    reduce_device_batch(ctx, ora, D.first_negative_blocks(), bids, tag="first negative")
    compare_state(ctx, ora, bids)
    ctx.close()


# (e) HDRF_SHA_CARRY is read once per process, so sha_chunk runs in one fresh child interpreter.
# Its timeout is a hang guard: 20 x the wall time of the same cases in-process, plus its start-up.
CHILD_CASES_S = 0.87          # child_cases() in-process on an MI355X (sha_carry), block generation included
CHILD_STARTUP_S = 20.0        # interpreter, numpy, library and HIP runtime load (0.4 s measured, warm)


def child_cases():
    case_sha_sweep(0)
    case_long(0)
    case_end_blocks()


@pytest.mark.gpu
def test_sha_chunk_kernel_child_process():
    """(e) HDRF_SHA_CARRY=0 (sha_chunk, the documented fallback): (a), (c) and (g) for hasher 0 in one
    child process, once; the timeout is only a hang guard."""
    env = dict(os.environ, HDRF_SHA_CARRY="0", PYTHONPATH=ROOT + os.pathsep + os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=20 * CHILD_CASES_S + CHILD_STARTUP_S)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "designed child ok, HDRF_SHA_CARRY=0" in r.stdout


if __name__ == "__main__":
    t0 = time.time()
    child_cases()
    print(f"designed child ok, HDRF_SHA_CARRY={os.environ.get('HDRF_SHA_CARRY', 'unset')}, "
          f"cases {time.time() - t0:.2f} s", flush=True)
