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
ranged reads across designed cuts).

The bookkeeping families ("Designed bookkeeping") pin where the chunker's speculate /
repair / stitch steps branch between segments: tests/lane_model.py predicts every segment's cut
counts, boundary outcome, jump and place in the block's offsets from the rule alone, the CPU tests
prove from it that each block reaches the branch it was built for (and stops reaching it when one
constant of the model is changed), and the GPU tests hold the chunker's own per-segment records
(hdrf_batch_seg_trace) to the model, besides the cuts, digests and stored bytes."""
import collections
import hashlib
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import designed as D
import lane_model as LM
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


# ---- CPU: the bookkeeping model (tests/lane_model.py) and the families built on it ----------------
K = LM.CONSTANTS


def _bookkeeping_blocks(seg):
    """[(tag, block, designed offsets)] of the bookkeeping families built for seg_len seg (family C apart)."""
    out = [("overrun_sweep",) + D.overrun_sweep(seg)[:2], ("overrun_edges",) + D.overrun_edges(seg)[:2]]
    out += [(f"small {i}",) + b for i, b in enumerate(D.small_blocks(seg))]
    out += [(f"repair d={d} hole={h}",) + D.repair_sweep(L, d, h)[:2] for (L, d) in D.REPAIR_SCRIPTS if L == seg
            for h in (False, True)]
    out += [(f"repair_bytes +{i}",) + b for i, b in enumerate(D.repair_bytes_blocks())]
    out += [(f"stitch give_up={g}",) + D.stitch_windows(seg, g)[:2] for g in (False, True)]
    return out


def test_model_constants_are_the_sources():
    assert {"kLaneOver", "kRepairBytes", "kRepairCuts", "kRqKeep", "kSegMaxWin", "kStitchNodes"} <= set(K)
    assert K["kRqKeep"] == D.RQ_KEEP and K["kStitchNodes"] == D.STITCH_NODES
    assert LM.default_params()["repair_bytes"] == K["kRepairBytes"] == 2 << 20
    # kRepairCuts cannot bind before kRepairBytes: that many cuts span more than the byte limit
    assert K["kRepairCuts"] * D.MIN_L > K["kRepairBytes"]
    # nor can the 64-entry lookup: a segment holds at most kSegMaxWin main cuts
    assert K["kSegMaxWin"] < 63 and max(D.SEG_LENS) == K["kSegMaxWin"] * D.MIN_L


@pytest.mark.parametrize("name", FAMILIES)
def test_model_offsets_equal_oracle(name):
    """Following the model's path through its own lists gives the reference's cuts, at both segment lengths."""
    for tag, blk, offs in _family(name):
        o = np.asarray(ora_chunk(blk))
        for seg in D.SEG_LENS:
            assert np.array_equal(model_of(blk, seg).offsets, o), f"{name} {tag} seg_len {seg}"


@pytest.mark.parametrize("seg", D.SEG_LENS)
def test_bookkeeping_cuts_designed_oracle_model(seg):
    for tag, blk, offs in _bookkeeping_blocks(seg):
        o = np.asarray(ora_chunk(blk))
        assert np.array_equal(o, offs), f"{tag}: the C oracle's cuts are not the designed ones"
        for s2 in D.SEG_LENS:
            assert np.array_equal(model_of(blk, s2).offsets, o), f"{tag}: the model's offsets at seg_len {s2}"
        if len(blk) < 400_000:
            assert pyref.chunking_closed_form(blk.tobytes()) == o.tolist(), f"{tag}: pyref.chunking_closed_form"


def test_coverage_steps_together():
    """The lanes step together: blocks of the sweeps hold boundaries whose shared cut the next segment
    had not made yet at that step, so the boundary is not a sync although the lists share the cut."""
    for seg, names in ((2808, ("chunk_sweep", "fallback_sweeps", "seams")), (14040, ("chunk_sweep", "long_search", "seams"))):
        for name in names:
            hits = [h for _, blk, _ in _family(name) for h in [model_of(blk, seg)] if h.passed_unseen()]
            assert hits, (seg, name)
            for m in hits:
                assert all(m.sync[k] < 0 or (m.sync[k] & 0xffff) > i for k, i, _ in m.passed_unseen())


def _sync(i, j):
    return i | (j << 16)


@pytest.mark.parametrize("seg", D.SEG_LENS)
def test_coverage_overrun(seg):
    """(A) from the model: syncs at overrun cut 1, 2, (3 | 7, 8) with j 0 and non-zero, at segments 62
    and 63; the cuts at e + seg_len - 1 and e + seg_len; the byte cap; 1- and 2-segment blocks; the
    last boundary."""
    blk, _, log = D.overrun_sweep(seg)
    m = model_of(blk, seg)
    got = set()
    for ev, a, _ in log[:-1]:
        assert m.on_path[a] and m.sync[a] == _sync(ev[1], ev[1]), (ev, a, m.state(a))
        assert m.over[a][ev[1]] == m.main[a + 1][ev[1]]
        got.add(ev[1] + 1)
    # 8 overrun cuts need 7 x 702 B = 4,914 B inside the next segment: more than 2,808
    assert got == ({1, 2, 3} if seg == 2808 else {1, 2, 3, 7, 8})
    assert {a for ev, a, _ in log if ev[0] == "sync"} >= {62, 63}
    assert any(m.sync[k] == _sync(1, 0) for k in range(m.nseg - 1))       # the plain lattice: j = 0 behind i = 1
    a = log[-1][1]                                                         # the chain that leaves for good
    assert m.sync[a] == LM.GIVEUP and m.n_over[a] == D.lattice_fail_cuts(seg, 351) and m.fallback and m.term == a
    assert m.repair_span[a] < K["kRepairBytes"] and len(m.ext[a]) < K["kRepairCuts"]   # the repair ran out of data
    assert m.rule.next((m.ext[a] or m.over[a])[-1], False) is None
    assert [model_of(b, seg).nseg for b, _ in D.small_blocks(seg)] == [1, 2, 3]
    m2 = model_of(D.small_blocks(seg)[1][0], seg)                           # the last boundary of a 2-segment block
    assert m2.state(0)[1:3] == ((4, LM.END) if seg == 2808 else (8, LM.GIVEUP))
    blk, _, where = D.overrun_edges(seg)
    m = model_of(blk, seg)
    e = {k: (a + 1) * seg for k, a in where.items()}
    a = where["last_byte"]
    assert m.sync[a] == _sync(0, 0) and m.over[a] == [e["last_byte"] + seg - 1] and m.on_path[a]
    a = where["last_byte_capped"]
    assert m.state(a)[1:6] == (0, LM.JUMP, 1, 0, 1) and m.ext[a] == [e["last_byte_capped"] + seg - 1]
    a = where["one_past"]
    c = e["one_past"] + seg
    assert m.over[a] == [c] and m.state(a)[2:6] == (LM.JUMP, 2, 0, 1) and m.over[a + 1][0] == c
    a = where["at_over_lim"]
    assert m.over[a] == [e["at_over_lim"] + seg - 64] and m.sync[a] == LM.JUMP and m.on_path[a]
    a = where["below_over_lim"]
    assert m.over[a][0] == e["below_over_lim"] + seg - 65 and m.n_over[a] == 2 and m.sync[a] == LM.JUMP


@pytest.mark.parametrize("seg", D.SEG_LENS)
def test_coverage_repairs(seg):
    """(B) from the model: the n_ext, jmp and jj values, an off-path repair beside an on-path one, a cut
    met only as another segment's overrun cut, kRepairBytes exactly and one byte more."""
    n_ext, jmp, jj_kind = set(), set(), set()
    for (L, d) in D.REPAIR_SCRIPTS:
        if L != seg:
            continue
        for hole in (False, True):
            blk, _, log = D.repair_sweep(L, d, hole)
            m = model_of(blk, seg)
            assert log[0][1] == (63 if hole else 62)
            for ev, a, tgt in log:
                assert m.on_path[a] and m.sync[a] == LM.JUMP and a + m.jmp[a] == tgt, (ev, a, m.state(a))
                assert m.ext_dst[a] >= 0 and m.n_over[a] == D.lattice_fail_cuts(seg, d)
                if hole:                                  # met at segment tgt - 1's overrun cut, matched one cut on
                    c = m.ext[a][-2]
                    assert c == tgt * seg + 1 == m.over[tgt - 1][0] and c not in m.main[tgt] and m.jj[a] == 0
                    continue
                assert m.n_ext[a] == ev[1]
                n_ext.add(ev[1])
                jmp.add(min(int(m.jmp[a]), 8))
                jj_kind |= {("first", "second")[j] for j in (0, 1) if m.jj[a] == j}
                if m.jj[a] == m.n_main[tgt] - 1:
                    jj_kind.add("last")
                if ev[1] >= 64:                           # the boundaries it passes over failed too: nothing to write
                    for b in (a + 1, a + 2):
                        assert not m.on_path[b] and m.sync[b] == LM.JUMP and m.n_ext[b] > 1 and m.ext_dst[b] == -1
    assert n_ext >= set(D.REPAIR_N_EXT) | {1}
    # jmp 1 needs a repair cut inside the next segment, which the lane walk records itself unless kLaneOver
    # stops it (14,040 only) or its search was capped (overrun_edges, last_byte_capped)
    assert jmp >= ({2, 3, 8} if seg == 2808 else {1, 2, 3, 8}) and jj_kind == {"first", "second", "last"}
    exact, past = (model_of(b, seg) for b, _ in D.repair_bytes_blocks())
    assert exact.state(0)[2:6] == (LM.JUMP, exact.ext[0][-1] // seg, 0, 3) and exact.repair_span[0] == K["kRepairBytes"]
    assert not exact.fallback and exact.over[0] == [] and exact.main[0] == [702, D.REPAIR_P0]
    assert past.sync[0] == LM.GIVEUP and past.repair_span[0] == K["kRepairBytes"] + 1 and past.fail_dst == 2


def test_coverage_queue_batch():
    """(C) from the model: failed boundaries >= kRqKeep + the surplus, short repairs, n_ext on the
    blocks' paths below and above 64."""
    blocks = D.queue_batch()
    ms = [model_of(b, 2808) for b, _ in blocks]
    assert sum(m.rq_count for m in ms) >= K["kRqKeep"] + D.QUEUE_SURPLUS
    assert sum(len(b) for b, _ in blocks) < 160_000_000 and max(len(b) for b, _ in blocks) <= 16 << 20
    for m in ms:
        on = [int(k) for k in m.failed if m.on_path[k]]
        ne = collections.Counter(m.n_ext[on].tolist())
        assert len(on) == m.rq_count and {1, 2, 64, 65, 66, 129} == set(ne) and ne[2] > 1000
        assert max(m.repair_span.values()) < K["kRepairBytes"] // 16 and not m.fallback


@pytest.mark.parametrize("give_up", [False, True])
@pytest.mark.parametrize("seg", D.SEG_LENS)
def test_coverage_stitch_windows(seg, give_up):
    """(D) from the model: more than two windows of irregular boundaries, on and off the path; jumps from
    the last node of a window to the first of the next; the path ends in the third window."""
    blk, _, log = D.stitch_windows(seg, give_up)
    m = model_of(blk, seg)
    N = K["kStitchNodes"]
    assert len(m.nodes) > 2 * N and sum(not m.on_path[k] for k in m.nodes) >= 16
    for w in (1, 2):
        src, dst = m.nodes[w * N - 1], m.nodes[w * N]
        assert m.on_path[src] and m.sync[src] == LM.JUMP and src + m.jmp[src] == dst and m.on_path[dst]
    t = m.term
    assert 2 * N <= m.node_index(t) < 3 * N and t == log[-1][1] and t < m.nseg - 1
    if give_up:
        assert m.sync[t] == LM.GIVEUP and m.fallback and m.fail_dst == int(m.piece.sum()) > 2 * N
    else:
        assert m.sync[t] == LM.END and not m.fallback and 0 < m.n_over[t] < D.lattice_fail_cuts(seg, 351)


def _changed(blk, seg, **params):
    """segments whose state a change of one model parameter changes, and the changed model"""
    a, b = model_of(blk, seg), LM.Model(blk, seg, **params)
    assert a.nseg == b.nseg
    return [k for k in range(a.nseg) if a.state(k)[:6] != b.state(k)[:6]], b


def test_teeth_each_block_sits_on_its_edge():
    """One constant of the model changed at a time: the prediction for the block built for that edge
    changes at the boundary built for it (no kernel is changed or run).  The final offsets never do:
    every branch leads to the same cuts, which is why only the trace can tell them apart."""
    # kLaneOver (8 overrun cuts do not fit in 2,808 B: 14,040 only)
    seg = 14040
    blk, offs, log = D.overrun_sweep(seg)
    at8 = [a for ev, a, _ in log if ev == ("sync", 7)]
    ch, m7 = _changed(blk, seg, lane_over=7)
    assert set(at8) <= set(ch) and all(m7.sync[a] == LM.JUMP for a in at8) and np.array_equal(m7.offsets, offs)
    ch, m9 = _changed(blk, seg, lane_over=9)
    assert not set(ch) & {a for ev, a, _ in log if ev[0] == "sync"}
    blk, offs, log = D.repair_sweep(seg, 351)
    a = log[0][1]                                       # n_ext 1: the 9th overrun cut would have been shared
    ch, m9 = _changed(blk, seg, lane_over=9)
    assert a in ch and m9.sync[a] == _sync(8, 8) and np.array_equal(m9.offsets, offs)
    # the lookup width: no list has 63 main cuts (kSegMaxWin = 20), so 63 changes nothing anywhere
    for s2 in D.SEG_LENS:
        for tag, b, _ in _bookkeeping_blocks(s2):
            if not tag.startswith("stitch"):
                assert _changed(b, s2, lookup=63)[0] == [], tag
                assert int(model_of(b, s2).n_main.max()) <= K["kSegMaxWin"]
    # kRepairBytes
    for seg in D.SEG_LENS:
        (exact, offs), (past, offs1) = D.repair_bytes_blocks()
        ch, lo = _changed(exact, seg, repair_bytes=K["kRepairBytes"] - 1)
        assert 0 in ch and lo.sync[0] == LM.GIVEUP and np.array_equal(lo.offsets, offs)
        assert 0 not in _changed(exact, seg, repair_bytes=K["kRepairBytes"] + 1)[0]
        ch, hi = _changed(past, seg, repair_bytes=K["kRepairBytes"] + 1)
        assert 0 in ch and hi.sync[0] == LM.JUMP and np.array_equal(hi.offsets, offs1)
        assert 0 not in _changed(past, seg, repair_bytes=K["kRepairBytes"] - 1)[0]
        # over_lim
        blk, offs, where = D.overrun_edges(seg)
        ch, up = _changed(blk, seg, over_lim_delta=16)
        assert where["at_over_lim"] in ch and up.n_over[where["at_over_lim"]] == 2 and np.array_equal(up.offsets, offs)
        assert where["last_byte_capped"] in ch and up.sync[where["last_byte_capped"]] == _sync(0, 0)
        ch, dn = _changed(blk, seg, over_lim_delta=-16)
        assert where["below_over_lim"] in ch and dn.n_over[where["below_over_lim"]] == 1 and np.array_equal(dn.offsets, offs)
        assert where["last_byte"] in ch and dn.sync[where["last_byte"]] == LM.JUMP and dn.n_over[where["last_byte"]] == 0


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


_MODELS = {}


def model_of(blk, seg_len):
    """the lane model of a (cached, read-only) designed block"""
    key = (blk.ctypes.data, len(blk), seg_len)
    if key not in _MODELS:
        _MODELS[key] = LM.Model(blk, seg_len)
    return _MODELS[key]


def check_trace(ctx, b, blk, seg_len, tag):
    """Block b of the batch just completed: the chunker's per-segment records equal the model's, every
    field of every segment (queue order is not part of them); -> the batch's repair-queue count."""
    m = model_of(blk, seg_len)
    tr, rq = ctx.batch_seg_trace(b, m.nseg)
    assert len(tr["sync"]) == m.nseg, f"{tag}: {len(tr['sync'])} segments, the model has {m.nseg}"
    want = dict(n_main=m.n_main, n_over=m.n_over, sync=m.sync, jmp=m.jmp, jj=m.jj, n_ext=m.n_ext, ext_dst=m.ext_dst,
                n_piece=m.piece)
    for f in ctx.SEG_TRACE_FIELDS:
        bad = np.flatnonzero(tr[f] != want[f])
        assert not len(bad), (f"{tag}: {f} differs from the model at segments {bad[:8].tolist()}: "
                              f"chunker {tr[f][bad[:8]].tolist()}, model {want[f][bad[:8]].tolist()}")
    assert np.array_equal(tr["n_piece"] > 0, m.on_path & (m.piece > 0)), f"{tag}: segments on the block's path"
    return rq


def reduce_blocks(ctx, ora, blocks, bid0, tag="", seg_len=None):
    """reduce_block of each (block, designed offsets) against the oracle; -> [(bid, block, offsets)].
    seg_len: the context's lane-walk segment length; the chunker's trace is then held to the model."""
    stored = []
    for i, (blk, offs) in enumerate(blocks):
        bid = bid0 + 7 * i
        g = ctx.reduce_block(blk, bid)
        if seg_len is not None:
            check_trace(ctx, 0, blk, seg_len, f"{tag} block {i}")
        o = ora.reduce(blk, bid)
        compare_block(g, o, tag=f"{tag} block {i}")
        if offs is not None:
            assert np.array_equal(g["offsets"], offs), f"{tag} block {i}: not the designed cuts"
        stored.append((bid, blk, g["offsets"]))
    return stored


def reduce_device_batch(ctx, ora, blocks, bids, fill=0, exact=False, tag="", seg_len=None):
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
    rq = [check_trace(ctx, i, blk, seg_len, f"{tag} batch block {i}") for i, (blk, _) in enumerate(blocks)] if seg_len else []
    ctx.dev_free(dev)
    return rq[0] if rq else None


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
SEG_OF = {1 << 16: 2808, None: 14040}


def _chunker_ctx(seg):
    kw = dict(CFG) if seg is None else dict(CFG, segment_bytes=seg)
    return Context(**kw), Oracle()


@pytest.mark.gpu
@pytest.mark.parametrize("seg", SEGS)
@pytest.mark.parametrize("group", ["sweeps", "long", "fallback", "seams", "interleaved"])
def test_chunker_families(group, seg):
    """(f) the chunker's general path at designed cuts; the per-segment trace equals the lane model's
    (these blocks hold the boundaries where a lane passes a shared cut the next lane has not made yet)."""
    blocks = {"sweeps": lambda: [D.chunk_sweep(), D.threshold_sweep()],
              "long": lambda: [D.long_search(), D.long_threshold()],
              "fallback": lambda: [D.fallback_sweeps()],
              "seams": lambda: [D.seams(U) for U in (65536,) + D.SEG_LENS],
              "interleaved": lambda: [D.interleaved(s, rf) for s in IL_SPACINGS for rf in (None, 1 << 19)]}[group]()
    ctx, ora = _chunker_ctx(seg)
    stored = reduce_blocks(ctx, ora, blocks, 0x6000, tag=group, seg_len=SEG_OF[seg])
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


# ---- GPU: the bookkeeping families, cuts and trace -------------------------------------------------
BOOK_GROUPS = {
    # blocks built for both segment lengths run under each: a cut must be right wherever the seams fall
    "overrun": lambda seg: [b for L in D.SEG_LENS for b in [D.overrun_sweep(L)[:2], D.overrun_edges(L)[:2]] + D.small_blocks(L)],
    "repair": lambda seg: [D.repair_sweep(L, d, h)[:2] for (L, d) in D.REPAIR_SCRIPTS for h in (False, True)]
    + D.repair_bytes_blocks(),
    "stitch": lambda seg: [D.stitch_windows(seg, g)[:2] for g in (False, True)],
}


@pytest.mark.gpu
@pytest.mark.parametrize("group,hasher,seg", [(g, 1, s) for g in BOOK_GROUPS for s in SEGS] + [("repair", 0, 1 << 16)])
def test_chunker_bookkeeping(group, hasher, seg):
    """(A, B, D) every block of the family: the designed cuts, the oracle's block result and state, the
    stored bytes, and the chunker's per-segment trace (cut counts, sync / jmp / jj / n_ext, ext_dst, the
    offsets each segment contributed) equal to the lane model's for every segment.  SHA sees nothing
    new in these chunks, so hasher 0 runs the repair family alone, once."""
    blocks = BOOK_GROUPS[group](SEG_OF[seg])
    kw = dict(CFG, max_block_bytes=32 << 20, hasher=hasher)
    if seg is not None:
        kw["segment_bytes"] = seg
    ctx, ora = Context(**kw), Oracle(hasher=hasher)
    stored = reduce_blocks(ctx, ora, blocks, 0x8000, tag=group, seg_len=SEG_OF[seg])
    compare_state(ctx, ora, [s[0] for s in stored])
    check_stored(ctx, stored)
    ctx.close()


@pytest.mark.gpu
def test_chunker_queue_beyond_kept_entries():
    """(C) one batch of 8 blocks at seg_len 2,808 with 20,480 failed boundaries, all on their blocks'
    paths: the repair queue runs 4,096 entries past kRqKeep, so that many repairs (which ones is up to
    the queue's atomics) take the emit pass's second walk, n_ext below and above 64 among them, and the
    rest the kept cuts.  Every cut of every block is judged, and the trace against the model.
    Host side, measured on the CPU: generation 0.7 s, the oracle (chunking + SHA-224) 0.9 s, the models
    1.5 s for the 126.6 MB batch."""
    blocks = D.queue_batch()
    ctx = Context(hasher=1, **dict(CFG, segment_bytes=1 << 16))
    ora = Oracle(hasher=1)
    bids = [0x9000 + i for i in range(len(blocks))]
    rq = reduce_device_batch(ctx, ora, blocks, bids, tag="queue", seg_len=2808)
    print(f"repair queue: {rq} entries, kRqKeep {K['kRqKeep']}")
    assert rq == sum(model_of(b, 2808).rq_count for b, _ in blocks) and rq >= K["kRqKeep"] + 1024
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
