"""Designed-sequence corpus (tests/designed_lz.py): the LZ4, Snappy and LZO kernels pinned at chosen
matches, and their decoders at streams the in-house encoders never write.

The data-driven codec tests reach lz4.hip, snappy.hip and lzo.hip only through the matches eight
generators happen to produce.  Here every match start, length, distance, literal run, search attempt
index and table collision is placed (designed_lz.py says how), and every decoder element form, length
run and window-refill phase is written out by hand.

CPU tests: the oracle's parsed output is exactly each case's designed sequence list and round-trips
through the oracle's decoder; the coverage each family claims is asserted as complete sets; the
designed LZ4 inputs also go through the liblz4 comparison of test_lz4_liblz4.py and the designed
Snappy inputs through pyarrow's encoder; the hand-built decoder streams decode to the builder's
expected bytes through liblz4, pyarrow's Snappy and (LZO: the only decoder there is) the oracle.

GPU tests: every designed input through Context.stream_block_host, byte for byte against the
oracle's file and decoded back; every hand-built file through stream_file_decode / lz4_file_decode."""
import ctypes

import numpy as np
import pytest

import designed_lz as Z
from helpers import make_block
from oracle.oracle import (hadoop_lz4_stream, hadoop_stream, lz4_block, lz4_block_decode, lz4_block_modern,
                           lzo1x_1, lzo1x_decode, lzop_stream, snappy_raw, snappy_raw_decode)
from test_lz4 import _liblz4, _parse_sequences
from test_snappy import _elements

try:
    import pyarrow as pa
    HAVE_PA = pa.Codec.is_available("snappy")
except Exception:  # pragma: no cover
    HAVE_PA = False

LZ4_NAMES = list(Z.LZ4_FAMILIES)


def _last_match(parsed):
    return [s for s in parsed if s[1] is not None][-1]


# =================================================================================================
# CPU, part A: LZ4
# =================================================================================================
_LZ4_PARSED = {}


def lz4_parsed(name):
    """[(tag, input, designed sequences, facts, the oracle's parsed sequences)] (computed once)."""
    if name not in _LZ4_PARSED:
        _LZ4_PARSED[name] = [c + (_parse_sequences(lz4_block(c[1])),) for c in Z.LZ4_FAMILIES[name]()]
    return _LZ4_PARSED[name]


@pytest.mark.parametrize("name", LZ4_NAMES)
def test_lz4_oracle_output_is_the_designed_sequences(name):
    for tag, d, seqs, _, parsed in lz4_parsed(name):
        assert d.size <= Z.LZ4_MAX_IN
        assert parsed == seqs, f"{name} {tag}: designed {seqs[:6]}, oracle {parsed[:6]}"
        assert lz4_block_decode(lz4_block(d), d.size) == d.tobytes(), f"{name} {tag}: round trip"


@pytest.mark.parametrize("name", LZ4_NAMES)
def test_lz4_designed_inputs_equal_liblz4_under_its_rules(name):
    """The comparison of test_lz4_liblz4.py (the oracle under liblz4 >= 1.9's three rules against a
    real liblz4) over the designed inputs: its rules apply to every block of at most 261,100 bytes."""
    pytest.importorskip("pyarrow")
    from test_lz4_liblz4 import liblz4
    for tag, d, _, _ in Z.LZ4_FAMILIES[name]():
        assert lz4_block_modern(d) == liblz4(d.tobytes()), f"{name} {tag}"


def test_lz4_coverage_match_lengths():
    got = {"fast": set(), "general": set()}
    for tag, _, _, facts, parsed in lz4_parsed("match_lengths"):
        f = facts["finds"][-1]
        assert _last_match(parsed)[2] == f["ml"]
        got["fast" if f["fast"] else "general"].add(_last_match(parsed)[2])
        # where the match ends in the 256-byte extension windows (they start 64 bytes before the found
        # position on the fast path, at the match start on the general path)
        f["win_end"] = (f["ml"] + (64 if f["fast"] else 0)) % 256
    want = set(range(4, 25)) | {15 + 4 + k for k in (254, 255, 256, 509, 510, 511, 764, 765, 1019, 1020, 1021)}
    for path in got:
        assert want <= got[path] and max(got[path]) >= 64 * 510 + 19, path
        assert got[path] == set(Z.LZ4_ML_ALL)
        ends = {((ml + (64 if path == "fast" else 0)) // 256, (ml + (64 if path == "fast" else 0)) % 256)
                for ml in got[path]}
        for j in (1, 2):                           # window steps: the end at -1, 0, +1, +3, +4 around them
            assert {(j - 1, 255), (j, 0), (j, 1), (j, 3), (j, 4)} <= ends, (path, j)


def test_lz4_coverage_literal_runs():
    got = set()
    for tag, _, _, facts, parsed in lz4_parsed("literal_runs"):
        f = facts["finds"][-1]
        where = "ip<64" if f["ip"] < 64 else "mref<64" if f["mref"] < 64 else "both>=64"
        got.add((_last_match(parsed)[0], where))
        assert f["chain"] or f["fast"] == (where == "both>=64" and f["ip"] - (f["start"] - f["lit"]) <= 64)
    runs = (0, 1, 14, 15, 16, 64, 65, 15 + 254, 15 + 255, 15 + 256, 16334, 16335, 16336, 15 + 255 * 65)
    # ip < 64 is the block's first match: its literals are all the bytes before it, 1..62 of them
    want = {(r, w) for r in runs for w in ("mref<64", "both>=64")} | {(r, "ip<64") for r in runs if 1 <= r <= 62}
    assert got == want


def test_lz4_coverage_attempt_index():
    got = {}
    for tag, _, _, facts, parsed in lz4_parsed("attempt_index"):
        f = facts["finds"][-1]
        assert _last_match(parsed)[0] == 1 + sum(Z.lz4_step(j) for j in range(f["k"])), tag
        got[f["k"]] = Z.batch_of(f["k"], Z.LZ4_BATCHES)
    assert set(got) == set(range(141))
    assert set(got.values()) == {(b, l) for b, m in enumerate((8, 16, 32, 64, 64)) for l in range(m)
                                 if sum((8, 16, 32, 64, 64)[:b]) + l <= 140}
    assert Z.lz4_step(60) == 1 and Z.lz4_step(61) == 2


def test_lz4_coverage_catch_up():
    got = set()
    for tag, _, _, facts, parsed in lz4_parsed("catch_up"):
        f = facts["finds"][-1]
        assert _last_match(parsed) == (f["lit"], f["off"], f["back"] + 9), tag
        got.add((f["back"], "fast" if f["fast"] else "general", f["stop"]))
    want = {(b, "fast", "byte") for b in (0, 1, 3, 4, 62, 63)} | {(b, "fast", "anchor") for b in (1, 3, 4, 62, 64)} | \
        {(b, "general", "byte") for b in (63, 64, 65, 128, 150)} | {(b, "general", "anchor") for b in (128, 150)} | \
        {(b, "general", "zero") for b in (1, 3, 4, 44)}
    assert got == want          # what is left out, and why: designed_lz.lz4_catch_up


def test_lz4_coverage_distances():
    offs = {True: set(), False: set()}
    seams = set()
    for tag, d, _, facts, parsed in lz4_parsed("distances"):
        if tag.startswith("dist=65536"):
            assert parsed == [(d.size, None, 0)] and [p - c for p, c in facts["far"]] == [65536]
        elif tag.startswith("seam"):
            (p2, p1), = facts["far"]
            assert p2 - p1 == 65536 and facts["slots"][p2][0] == facts["slots"][p1][0]
            assert _last_match(parsed)[1] == facts["finds"][-1]["ip"] - p2 <= 65535
            seams.add((p2 >> 16, tag.split()[1]))
            B = int(tag.split()[0][5:])
            assert abs(p2 - B) < 4096
        else:
            offs[facts["u16"]].add(_last_match(parsed)[1])
    assert offs[False] == {1, 2, 3, 4, 255, 256, 65534, 65535} and offs[True] == {1, 2, 3, 4, 255, 256}
    # below the first seam no position has one 65,536 bytes before it
    assert seams == {(1, "above"), (2, "above"), (3, "above"), (1, "below"), (2, "below")}


def test_lz4_coverage_equal_hashes():
    """The oracle's output cannot show that the kernel's replay path ran: "same batch, same index" is
    asserted from the builder's model of the schedule (the sequences themselves by the test above)."""
    cases = {c[0]: c for c in lz4_parsed("equal_hashes")}
    assert set(cases) == {f"{k} {t}" for k in ("none tags=equal", "none tags=different", "known", "undo")
                          for t in ("byU16", "byU32")}
    for tab in ("byU16", "byU32"):
        for tags in ("equal", "different"):
            _, d, _, facts, _ = cases[f"none tags={tags} {tab}"]
            assert facts["u16"] == (tab == "byU16") == (d.size < 65547)
            a, b = facts["slots"][81], facts["slots"][86]
            assert a[0] == b[0] and (a[1] == b[1]) == (tags == "equal")
            assert Z.batch_of(81 - 71, Z.LZ4_BATCHES)[0] == Z.batch_of(86 - 71, Z.LZ4_BATCHES)[0] == 1
        f = cases[f"known {tab}"][3]["finds"][-1]
        assert Z.batch_of(f["k"], Z.LZ4_BATCHES)[0] == Z.batch_of(f["mref"] - 71, Z.LZ4_BATCHES)[0] == 1
        _, _, seqs, facts, _ = cases[f"undo {tab}"]
        s = facts["slots"]
        assert s[20][0] == s[85][0] == s[90][0] == s[94][0] and s[90][1] == s[20][1] != s[94][1]
        assert [Z.batch_of(p - 71, Z.LZ4_BATCHES)[0] for p in (79, 85, 90, 94)] == [1, 1, 1, 1]
        assert seqs[1:3] == [(9, 40, 5), (1, 65, 4)]


def test_lz4_coverage_chains_and_block_ends():
    got = set()
    for tag, _, _, facts, parsed in lz4_parsed("chains"):
        if tag.startswith("chain"):
            i = next(i for i, s in enumerate(parsed) if s[0] == 0 and s[1] is not None)
            slots, ip = facts["slots"], facts["finds"][1]["ip"]
            got.add((parsed[i - 1][2] % 256, parsed[i][1] == 2, slots[ip - 2][0] == slots[ip][0]))
        else:
            assert all(s[0] != 0 for s in parsed[1:-1])
            s = facts["slots"]
            assert s[70][0] == s[20][0] and s[70][1] == s[20][1] and s[70][2] == 20     # index, tag, candidate
    # first match length mod 256 (0: ends at a window start, 255: one byte before), source ip - 2, h2 == h0
    assert got == {(m, a, a) for m in (30, 255, 0, 1) for a in (True, False)}
    ends = {c[0]: c[4] for c in lz4_parsed("block_ends")}
    n = 200
    assert [ends[f"n={k}"] for k in (12, 13, 14)] == [[(k, None, 0)] for k in (12, 13, 14)]
    assert ends["match into the last 5 bytes"] == [(60, 52, n - 65), (5, None, 0)]
    assert [ends[f"match ends at mflimit{e:+d}"][-1][0] for e in (-1, 0, 1)] == [13, 12, 11]
    assert ends["copy planted at n-13"][-2:] == [(37, 68, 6), (7, None, 0)]
    assert ends["copy planted at n-12"][-1] == ends["copy planted at n-10"][-1] == (50, None, 0)


# =================================================================================================
# CPU, part A: Snappy
# =================================================================================================
SN_NAMES = list(Z.SN_FAMILIES)
_PARSED = {}


def sn_parsed(name):
    if ("sn", name) not in _PARSED:
        _PARSED["sn", name] = [c + (_elements(snappy_raw(c[1])),) for c in Z.SN_FAMILIES[name]()]
    return _PARSED["sn", name]


def lzo_parsed(name):
    if ("lzo", name) not in _PARSED:
        _PARSED["lzo", name] = [c + (Z.lzo_parse(lzo1x_1(c[1])),) for c in Z.LZO_FAMILIES[name]()]
    return _PARSED["lzo", name]


@pytest.mark.parametrize("name", SN_NAMES)
def test_snappy_oracle_output_is_the_designed_elements(name):
    for tag, d, els, _, (raw, parsed) in sn_parsed(name):
        assert d.size <= (2 * Z.SN_FRAG if tag == "two fragments" else Z.SN_FRAG)
        assert raw == d.size and parsed == els, f"{name} {tag}: designed {els[:6]}, oracle {parsed[:6]}"
        c = snappy_raw(d)
        assert snappy_raw_decode(c, d.size) == d.tobytes(), f"{name} {tag}: round trip"
        if HAVE_PA:                                # an encoder the project did not write
            assert c == pa.compress(d.tobytes(), codec="snappy", asbytes=True), f"{name} {tag}: pyarrow's encoder"


def test_snappy_coverage_copies_and_offsets():
    got, pieces = set(), {}
    for tag, _, _, facts, (_, parsed) in sn_parsed("copy_lengths"):
        f = facts["finds"][-1]
        cp = [(k, ln) for k, ln, off in parsed if k != "lit"]
        assert sum(ln for _, ln in cp) == f["ml"] and {off for k, _, off in parsed if k != "lit"} == {f["off"]}
        got.add((f["ml"], f["off"]))
        pieces[f["ml"], f["off"]] = cp
    lens = set(range(4, 14)) | {59, 60, 61, 63, 64, 65, 66, 67, 68, 69, 71, 72, 127, 128, 131, 132, 133, 64 * 65 + 68}
    assert {l for l, _ in got} == lens | set(Z.SN_COPY_WINDOW) and got == {(l, o) for l, _ in got for o in (2047, 2048)}
    assert pieces[11, 2047] == [("c1", 11)] and pieces[11, 2048] == [("c2", 11)] and pieces[12, 2047] == [("c2", 12)]
    assert pieces[64, 2048] == [("c2", 64)] and pieces[65, 2047] == [("c2", 60), ("c1", 5)]
    assert pieces[67, 2048] == [("c2", 60), ("c2", 7)] and pieces[68, 2047] == [("c2", 64), ("c1", 4)]
    assert pieces[64 * 65 + 68, 2048] == [("c2", 64)] * 66 + [("c2", 4)]          # more than 64 pieces of 64
    offs = {f["finds"][-1]["off"] for _, _, _, f, _ in sn_parsed("offsets")}
    assert offs == {1, 2, 3, 4, 255, 256, 2047, 2048, 32767, 32768, 65519, 65518, 65517}
    # 65,519 is the largest: the last examined position is n - 15 - 1 and byte 0 is never in the table
    assert [p for _, p in Z.SnappyDesign(Z.SN_FRAG, 0).schedule()][-1] <= Z.SN_FRAG - 16


def test_snappy_coverage_literals_attempts_sizes_ends():
    tails = {parsed[-1][1] for _, _, _, _, (_, parsed) in sn_parsed("literals") if parsed}
    assert tails == {1, 59, 60, 61, 255, 256, 257, 65536, 14, 15, 16}
    assert {c[1].size for c in sn_parsed("literals")} >= {0, 1, 14, 15, 16, 65536}
    ks = {}
    for tag, _, _, facts, (_, parsed) in sn_parsed("attempt_index"):
        if tag.startswith("attempt"):
            k = facts["finds"][-1]["k"]
            ks[k] = Z.batch_of(k, Z.SN_BATCHES)
    assert set(ks) == set(range(141)) and set(ks.values()) == \
        {(b, l) for b, m in enumerate((16, 32, 64, 64)) for l in range(m) if sum((16, 32, 64, 64)[:b]) + l <= 140}
    eq = {c[0]: c for c in sn_parsed("attempt_index") if c[0].startswith("equal")}
    s = eq["equal index: none"][3]["slots"]
    assert s[32][0] == s[38][0] and Z.batch_of(32 - 29, Z.SN_BATCHES)[0] == Z.batch_of(38 - 29, Z.SN_BATCHES)[0] == 0
    f = eq["equal index: known"][3]["finds"][-1]
    assert (f["src"], f["ip"]) == (32, 38)
    s = eq["equal index: undo"][3]["slots"]
    assert s[10][0] == s[34][0] == s[39][0] == s[43][0]
    assert {Z.batch_of(p - 29, Z.SN_BATCHES)[0] for p in (29, 34, 39, 43)} == {0}
    assert eq["equal index: undo"][2][:6] == [("lit", 20, 0), ("c1", 8, 15), ("lit", 1, 0), ("c1", 4, 14),
                                              ("lit", 1, 0), ("c1", 4, 24)]
    sizes = {c[1].size for c in sn_parsed("fragment_sizes") if c[0] != "two fragments"}
    assert sizes == {s for k in range(8, 17) for s in ((1 << k) - 1, 1 << k, (1 << k) + 1) if s <= 65536}
    assert {f["mask"] for c in sn_parsed("fragment_sizes") for f in [c[3]]} == {(1 << k) - 1 for k in range(8, 16)}
    two = next(c for c in sn_parsed("fragment_sizes") if c[0] == "two fragments")
    assert two[1].size == 65536 + 300 and two[1][65536 + 40:65536 + 60].tobytes() == two[1][65436:65456].tobytes()
    ends = {300 - f["finds"][-1]["ip"] - f["finds"][-1]["ml"] for _, _, _, f, _ in sn_parsed("match_ends")}
    assert ends == {0, 1, 2, 3, 4, 14, 15, 16}     # n .. n - 4, lim + 1, lim, lim - 1


# =================================================================================================
# CPU, part A: LZO (the oracle is the only encoder and the only decoder)
# =================================================================================================
LZO_NAMES = list(Z.LZO_FAMILIES)


@pytest.mark.parametrize("name", LZO_NAMES)
def test_lzo_oracle_output_is_the_designed_instructions(name):
    for tag, d, els, _, parsed in lzo_parsed(name):
        assert parsed == els, f"{name} {tag}: designed {els[-6:]}, oracle {parsed[-6:]}"
        assert np.array_equal(lzo1x_decode(lzo1x_1(d), d.size), d), f"{name} {tag}: round trip"


def test_lzo_coverage():
    last = [[e for e in p if e[0] != "lit"][-1] for *_, p in lzo_parsed("class_edges")]
    assert {(c, ln, d) for c, d, ln in last} == \
        {("M2", 8, 2048), ("M3", 9, 2048), ("M3", 8, 2049), ("M3", 9, 2049), ("M3", 10, 16384), ("M4", 10, 16385)} | \
        {("M3", ln, 3000) for ln in (33, 34, 288, 289, 543, 544)} | {("M4", ln, 20000) for ln in (9, 10, 264, 265)} | \
        {("M4", 12, d) for d in (32767, 32768, 32769)}
    runs, trail = set(), set()
    for tag, _, _, facts, p in lzo_parsed("literal_runs"):
        i = max(i for i, e in enumerate(p) if e[0] != "lit")
        t = p[i - 1][1] if p[i - 1][0] == "lit" else 0
        assert t == facts["finds"][-1]["lit"]
        if "after" in tag:
            trail.add((t, p[i - 2][0]))
        else:
            runs.add(t)
    assert runs == {0, 1, 2, 3, 4, 18, 19, 18 + 255, 18 + 256, 18 + 510, 18 + 511}
    assert trail == {(t, c) for t in (1, 2, 3) for c in ("M2", "M3", "M4")}
    first = {c[1].size: c[4] for c in lzo_parsed("first_literals")}
    assert set(first) == {0, 1, 20, 21, 31, 32, 237, 238, 239, 1000}
    assert all(first[n] == ([("lit", n, "first")] if n else []) for n in (0, 1, 20, 21, 31, 32, 237, 238))
    assert first[239] == [("lit", 239, "run")] and first[1000] == [("lit", 1000, "run")]
    assert len(lzo1x_1(lzo_parsed("first_literals")[-1][1])) >= 1000             # does not shrink: stored raw
    gaps, opened = set(), set()
    for tag, d, _, facts, p in lzo_parsed("extension_ends"):
        f = facts["finds"][-1]
        (opened if tag.startswith("open") else gaps).add(f["ip_end"] - f["end"])
    assert gaps == {0, 1, 7, 8, 9} and opened == {-k for k in range(8)}            # done: 0..7 bytes past ip_end
    seams = {c[0]: c for c in lzo_parsed("seams")}
    for tail in (21, 23, 400):
        c = seams[f"carry 9, last sub-block {tail}"]
        assert c[3]["finds"][-1 if tail != 400 else -2]["end"] == 49152 - 9
        assert c[4][-1] == (("lit", 9 + tail, "run") if tail != 400 else c[4][-1])
    assert ("lit", 9 + 30, "run") in seams["carry 9, last sub-block 400"][4]
    assert seams["carry a whole sub-block, source across the seam"][4][:2] == [("lit", 49152 + 30, "run"), ("M3", 20, 12)]


# =================================================================================================
# CPU, part B: the hand-built decoder streams against decoders the project did not write
# =================================================================================================
def test_lz4_streams_decode_through_liblz4():
    L = _liblz4()
    for fam in (Z.lz4_straddle_blocks, Z.lz4_element_blocks):
        for b in fam():
            tag, blk, raw = b[:3]
            assert raw.size <= Z.LZ4_MAX_IN and lz4_block_decode(blk, raw.size) == raw.tobytes(), tag
            if L is not None:
                out = ctypes.create_string_buffer(raw.size)
                assert L.LZ4_decompress_safe(blk, out, len(blk), raw.size) == raw.size and out.raw == raw.tobytes(), tag
    if L is None:
        pytest.skip("liblz4 not present: checked with the oracle's decoder only")


def test_lz4_stream_coverage():
    starts = set()
    for tag, blk, raw in Z.lz4_straddle_blocks()[:-1]:
        L0 = int(tag.split("=")[1])
        starts.add(1 + 33 + L0)                    # the token, 33 length bytes, the literal
    assert set(range(Z.DEC_WIN - 24, Z.DEC_WIN + 25)) <= starts
    assert {s % 16 for s in starts if s >= Z.DEC_WIN} == set(range(16))
    assert len(Z.lz4_straddle_blocks()[-1][1]) > 3 * Z.DEC_WIN
    seqs = [s for b in Z.lz4_element_blocks() for s in b[3]]
    for off in (1, 2, 3, 4, 63, 64, 65, 65535):
        mls = {ml for _, o, ml in seqs if o == off}
        assert {4, 18, 19, 19 + 254, 19 + 255, 70000} <= mls
        assert {m for m in (off - 1, off, off + 1) if m >= 4} <= mls
    assert Z.lz4_element_blocks()[-1][2].size == 261100 and len(_parse_sequences(Z.lz4_element_blocks()[-1][1])) == 1


@pytest.mark.skipif(not HAVE_PA, reason="pyarrow snappy not importable")
def test_snappy_streams_decode_through_pyarrow():
    for fam in (Z.snappy_straddle_blocks, Z.snappy_element_blocks):
        for b in fam():
            tag, blk, raw = b[:3]
            assert raw.size <= Z.SNAPPY_MAX_IN and snappy_raw_decode(blk, raw.size) == raw.tobytes(), tag
            assert pa.decompress(blk, decompressed_size=raw.size, codec="snappy", asbytes=True) == raw.tobytes(), tag


def test_snappy_stream_coverage():
    starts = {k: set() for k in Z.SN_STRADDLE_KINDS}
    for tag, blk, raw in Z.snappy_straddle_blocks()[:-1]:
        n, els = _elements(blk)
        assert n == raw.size and len(els) == 3
        starts[tag.split()[0]].add(2 + 3 + els[0][1])     # 2 varint bytes, tag + 2 length bytes, the literal
    for k, s in starts.items():
        assert set(range(Z.DEC_WIN - 24, Z.DEC_WIN + 25)) <= s, k
    copies = set()
    for _, blk, raw, elems in Z.snappy_element_blocks():
        assert [(k, ln, off) for k, ln, off in _elements(blk)[1] if k != "lit"] == [e for e in elems if e[0] != "lit"]
        copies |= {e for e in elems if e[0] != "lit"}
    for kind, lens, top in (("c1", range(4, 12), 2047), ("c2", range(1, 65), 65535), ("c4", range(1, 65), 1 << 31)):
        for ln in lens:
            want = {o for o in (1, 2, 3, ln - 1, ln, ln + 1, 2047, 2048, 65535, 65536, 200000) if 1 <= o <= top}
            assert {o for k, l, o in copies if k == kind and l == ln} == want, (kind, ln)


def test_lzo_streams_decode_through_the_oracle():
    """lzo1x_decode is the only LZO decoder on the test machines; the parse below is the builder's."""
    seen = set()
    for tag, blk, raw, log in Z.lzo_element_blocks():
        assert np.array_equal(lzo1x_decode(blk, raw.size), raw), tag
        assert [e[:2] for e in Z.lzo_parse(blk)] == [e[:2] for e in log], tag
        seen |= {e for e in Z.lzo_parse(blk)}
    m = {k: {(d, l) for kk, d, l in seen if kk == k} for k in ("M1", "M2", "M3", "M4")}
    assert m["M1"] == {(2049, 3), (3072, 3), (1, 2), (1024, 2)}
    assert {(1, 3), (2048, 8), (1, 8), (2048, 3)} <= m["M2"]
    assert {l for _, l in m["M3"]} >= {3, 33, 34, 288, 289, 543, 544} and {d for d, _ in m["M3"]} >= {1, 2, 3, 2049, 16384}
    assert {l for _, l in m["M4"]} >= {3, 9, 10, 264, 265} and {d for d, _ in m["M4"]} == {16385, 32767, 32768, 32769, 49151}
    assert {(n, f) for k, n, f in seen if k == "lit" and f == "first"} == {(t, "first") for t in (1, 3, 4, 238)}
    assert {n for k, n, f in seen if k == "lit" and f == "trail"} == {1, 2, 3}
    assert {n for k, n, f in seen if k == "lit" and f == "run"} >= {4, 18, 19, 273, 274, 528, 529}
    assert any(d < l for k, d, l in seen if k in ("M2", "M3") and d in (1, 2, 3))


# =================================================================================================
# GPU
# =================================================================================================
def _lz4_spans(seqs):
    """[(first byte, one past the last byte)] of each designed sequence in the encoded block."""
    out, p = [], 0

    def ext(v):
        return 0 if v < 15 else 1 + (v - 15) // 255
    for lit, off, ml in seqs:
        q = p + 1 + ext(lit) + lit + (0 if off is None else 2 + ext(ml - 4))
        out.append((p, q))
        p = q
    return out


def _explain(what, tag, got, want, head, seqs, spans):
    """The failure message: family and case, the first differing byte, the designed sequence it is in."""
    if got == want:
        return None
    n = min(len(got), len(want))
    i = next((i for i in range(n) if got[i] != want[i]), n)
    k = next((k for k, (a, b) in enumerate(spans) if a <= i - head < b), None)
    return (f"{what} {tag}: file byte {i} (block byte {i - head}) is "
            f"{got[i] if i < len(got) else 'missing'}, reference {want[i] if i < len(want) else 'missing'}; "
            f"lengths {len(got)} / {len(want)}; designed sequence {k}: {seqs[k] if k is not None else None}")


@pytest.fixture(scope="module")
def ctx():
    from hdrf_amd.lib import Context
    c = Context(max_block_bytes=1 << 20, max_batch_blocks=1, index_log2=16, arena_slots=8)
    c.set_lzop_mtime(1234567)
    yield c
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", LZ4_NAMES)
def test_gpu_lz4_designed_blocks_match_oracle(ctx, name):
    """One call per designed input (each a single write of at most 261,100 bytes: one LZ4 block)."""
    for tag, d, seqs, _ in Z.LZ4_FAMILIES[name]():
        want = hadoop_lz4_stream(d, [d.size])
        assert int.from_bytes(want[:4], "big") == d.size and int.from_bytes(want[4:8], "big") == len(want) - 8
        got = ctx.stream_block_host(4, 1, d, [d.size])
        msg = _explain(f"lz4 {name}", tag, got, want, 8, seqs, _lz4_spans(seqs))
        assert msg is None, msg
        assert ctx.stream_file_decode(4, got, d.size) == d.tobytes(), f"lz4 {name} {tag}: read back"


def _sn_spans(els, n):
    out, p = [], len(Z._varint(n))
    for k, ln, _ in els:
        q = p + (2 if k == "c1" else 3 if k == "c2" else 1 + ln + (0 if ln <= 60 else ((ln - 1).bit_length() + 7) // 8))
        out.append((p, q))
        p = q
    return out


def _lzo_spans(els):
    out, p = [], 0
    for e in els:
        if e[0] == "lit":
            q = p + e[1] + {"first": 1, "trail": 0}.get(e[2], 1 if e[1] <= 18 else 2 + (e[1] - 19) // 255)
        else:
            lim = {"M3": 33, "M4": 9}.get(e[0])
            q = p + (2 if lim is None else 3 if e[2] <= lim else 4 + (e[2] - lim - 1) // 255)
        out.append((p, q))
        p = q
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", SN_NAMES)
def test_gpu_snappy_designed_fragments_match_oracle(ctx, name):
    """One call per designed input (a single write of at most 218,422 bytes: one raw snappy buffer)."""
    for tag, d, els, _ in Z.SN_FAMILIES[name]():
        w = [d.size] if d.size else []
        want = hadoop_stream(0, d, w)
        if d.size:
            assert int.from_bytes(want[:4], "big") == d.size and int.from_bytes(want[4:8], "big") == len(want) - 8
        got = ctx.stream_block_host(0, 1, d, w)
        msg = _explain(f"snappy {name}", tag, got, want, 8, els, _sn_spans(els, d.size))
        assert msg is None, msg
        assert ctx.stream_file_decode(0, got, d.size) == d.tobytes(), f"snappy {name} {tag}: read back"


@pytest.mark.gpu
@pytest.mark.parametrize("name", LZO_NAMES)
def test_gpu_lzo_designed_blocks_match_oracle(ctx, name):
    """One call per designed input (a single write of at most 245,693 bytes: one lzop block)."""
    for tag, d, els, _ in Z.LZO_FAMILIES[name]():
        w = [d.size] if d.size else []
        want = bytes(lzop_stream(d, w, mtime=1234567))
        head = 9 + 25 + 4 + 8
        if d.size:
            assert int.from_bytes(want[head - 8:head - 4], "big") == d.size and \
                int.from_bytes(want[head - 4:head], "big") == len(want) - head - 4
        got = ctx.stream_block_host(3, 1, d, w)
        msg = _explain(f"lzo {name}", tag, got, want, head, els, _lzo_spans(els))
        assert msg is None, msg
        assert ctx.stream_file_decode(3, got, d.size) == d.tobytes(), f"lzo {name} {tag}: read back"


def _first_diff(got, want, where, tags):
    got = np.frombuffer(got, np.uint8)
    if got.size == want.size and np.array_equal(got, want):
        return None
    n = min(got.size, want.size)
    bad = np.nonzero(got[:n] != want[:n])[0]
    i = int(bad[0]) if bad.size else n
    k = max(j for j, (_, o) in enumerate(where) if o <= i) if where else 0
    return f"decoded byte {i} differs (sizes {got.size} / {want.size}): block {k} ({tags[k]}), its byte {i - where[k][1]}"


def _check_residues(where):
    """The blocks' start offsets in the file and in the output reach every residue mod 16."""
    assert {a % 16 for a, _ in where} == set(range(16)) and {o % 16 for _, o in where} == set(range(16))


@pytest.mark.gpu
@pytest.mark.parametrize("fam", ["lz4_straddle_blocks", "lz4_element_blocks"])
def test_gpu_lz4_decoder_hand_built_streams(ctx, fam):
    blocks = getattr(Z, fam)()
    f, raw, where = Z.frame_groups([b[1:3] for b in blocks])
    if fam == "lz4_straddle_blocks":
        _check_residues(where)
    tags = [b[0] for b in blocks]
    for call in (lambda: ctx.stream_file_decode(4, f, raw.size), lambda: ctx.lz4_file_decode(f, raw.size)):
        msg = _first_diff(call(), raw, where, tags)
        assert msg is None, f"{fam}: {msg}"


@pytest.mark.gpu
@pytest.mark.parametrize("fam", ["snappy_straddle_blocks", "snappy_element_blocks"])
def test_gpu_snappy_decoder_hand_built_streams(ctx, fam):
    blocks = getattr(Z, fam)()
    f, raw, where = Z.frame_groups([b[1:3] for b in blocks])
    if fam == "snappy_straddle_blocks":
        _check_residues(where)
    msg = _first_diff(ctx.stream_file_decode(0, f, raw.size), raw, where, [b[0] for b in blocks])
    assert msg is None, f"{fam}: {msg}"


@pytest.mark.gpu
def test_gpu_lzo_decoder_hand_built_streams(ctx):
    blocks = Z.lzo_element_blocks()
    header = bytes(lzop_stream(np.zeros(0, np.uint8), []))[:-4]
    f, raw, where = Z.frame_lzop(header, [b[1:3] for b in blocks])
    msg = _first_diff(ctx.stream_file_decode(3, f, raw.size), raw, where, [b[0] for b in blocks])
    assert msg is None, f"lzo elements: {msg}"


def _lz4_hc():
    try:
        L = ctypes.CDLL("liblz4.so.1")
        L.LZ4_compress_HC.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_int]
        L.LZ4_compress_HC.restype = ctypes.c_int
        return L
    except (OSError, AttributeError):
        return None


def hc_blocks():
    L = _lz4_hc()
    out = []
    for kind in ("random", "zeros", "ff", "text", "lowent", "periodic", "sparse", "binary"):
        for n in (70000, 261100):
            d = make_block(kind, 31 + n, n)
            buf = ctypes.create_string_buffer(n + n // 255 + 16)
            c = L.LZ4_compress_HC(d.tobytes(), buf, n, len(buf), 9)
            assert c > 0
            out.append((f"HC {kind} {n}", buf.raw[:c], d))
    return out


def test_lz4_hc_parses_differ_from_r123():
    if _lz4_hc() is None:
        pytest.skip("liblz4 (LZ4_compress_HC) not present")
    for tag, blk, d in hc_blocks():
        assert lz4_block_decode(blk, d.size) == d.tobytes(), tag
        if "text 261100" in tag:
            assert len(_parse_sequences(blk)) > 100 * len(_parse_sequences(lz4_block(d)))


@pytest.mark.gpu
def test_gpu_lz4_decoder_foreign_encoder(ctx):
    """Blocks written by liblz4's high-compression encoder (level 9): other parses than r123's."""
    if _lz4_hc() is None:
        pytest.skip("liblz4 (LZ4_compress_HC) not present")
    blocks = hc_blocks()
    f, raw, where = Z.frame_groups([b[1:3] for b in blocks])
    msg = _first_diff(ctx.stream_file_decode(4, f, raw.size), raw, where, [b[0] for b in blocks])
    assert msg is None, f"LZ4 HC: {msg}"
