"""Seek tables (hdrf_seek_build / _drop / _info_get), the seek path of hdrf_read_batch / hdrf_read_range and
the verified ranged reads.  The expected bytes of every read are slices of the test's own blocks (or of the
containers the test tampered with itself), never a second read through the code under test."""
import ctypes
import hashlib
import os
import subprocess

import numpy as np
import pytest

from hdrf_amd.lib import READ_MAX_REQS, Context, HdrfError, ReadReq, SeekInfo, load
from test_gc import CIDS, SMALL, build, enc_value, hand_store
from test_read_batch import (FILL, GUARD, MISALIGN, PARAMS, Store, dec_value, forced_cut_blocks, ranges_of, serve,
                             store_blocks)

gpu = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVAL, NOTFOUND, UNSUPPORTED, CORRUPT = -1, -5, -6, -8
HASH = {0: hashlib.sha1, 1: hashlib.sha224}


# ---- CPU: the ABI and the host-side plan -------------------------------------------------------
def test_seek_info_size_matches_the_c_static_assert():
    assert ctypes.sizeof(SeekInfo) == 40
    src = open(os.path.join(ROOT, "hdrf_amd", "csrc", "api_seek.hip")).read()
    assert "static_assert(sizeof(hdrf_seek_info) == 40" in src


def test_null_arguments_are_invalid():
    L = load()
    ids = (ctypes.c_uint64 * 1)(1)
    res = (ctypes.c_int32 * 1)()
    one = (ReadReq * 1)()
    bad = (ctypes.c_int64 * 1)()
    info = SeekInfo()
    assert L.hdrf_seek_build(None, ids, 1, res) == INVAL
    assert L.hdrf_seek_build(None, None, 0, None) == INVAL
    assert L.hdrf_seek_drop(None, None, 0) == INVAL
    assert L.hdrf_seek_info_get(None, ctypes.byref(info)) == INVAL
    assert L.hdrf_read_batch_verified(None, 1, one, bad) == INVAL
    assert L.hdrf_read_range_verified(None, 1, 0, 10, None, 0, bad) == INVAL


def test_seek_plan_under_asan_and_ubsan(tmp_path):
    """tests/cpp/seek_plan_test.cpp: the span and the row bound against a per-byte model, the build's groups
    and the scratch layout, as a plain program built with -fsanitize=address,undefined."""
    exe = str(tmp_path / "seek_plan_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "seek_plan_test.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "PASS" in r.stdout


# ---- the stores and the model of what a call probes --------------------------------------------
_cache = {}


def _store(kind, hasher, compressor):
    key = (kind, hasher, compressor)
    if key not in _cache:
        if kind == "main":
            _cache[key] = Store(hasher, compressor, store_blocks(), 5000)
        else:
            _cache[key] = Store(hasher, compressor, forced_cut_blocks(), 6000, container_max=1 << 21)
    return _cache[key]


@pytest.fixture(scope="module")
def stores():
    yield _store
    for s in _cache.values():
        s.close()
    _cache.clear()


def clip(size, off, length):
    return max(0, min(length, size - off))


def row_bound(lens, clen):
    """seek_row_bound over a recipe's chunk lengths: the rows a request with a table is given."""
    n = len(lens)
    if clen == 0:
        return 0
    minlen = min(lens[:-1]) if n > 1 else 1 << 32
    return n if minlen == 0 else min(n, clen // minlen + 2)


def chunks_under(lens, off, clen):
    """Chunks that share a byte with [off, off + clen), by walking the recipe."""
    pos, hit = 0, 0
    for n in lens:
        hit += clen > 0 and n > 0 and pos < off + clen and pos + n > off
        pos += n
    return hit


def check_rows(ctx, reqs, lens_of, sizes, tabled):
    """What hdrf_seek_info reports of the call that served reqs = [(block, off, length), ...]."""
    info = ctx.seek_info()
    want_rows = under = 0
    for blk, off, length in reqs:
        lens = lens_of[blk]
        clen = clip(sizes[blk], off, length)
        want_rows += row_bound(lens, clen) if blk in tabled else len(lens)
        under += chunks_under(lens, off, clen)
    assert info["last_seek_reqs"] == sum(blk in tabled for blk, _, _ in reqs)
    assert info["last_rows"] == want_rows and (not tabled or under <= want_rows), (info, want_rows, under)
    return info


# ---- GPU ---------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("hasher,compressor", PARAMS)
@pytest.mark.parametrize("kind", ["main", "forced-cut"])
def test_ranges_equal_slices_from_tables(stores, kind, hasher, compressor):
    s = stores(kind, hasher, compressor)
    ctx = s.ctx
    lens_of = {i: [n for _, _, n in s.chunks[i]] for i in s.ids}
    sizes = {i: len(s.blocks[i]) for i in s.ids}
    ctx.seek_drop(None)
    assert ctx.seek_info()["bytes"] == 0 and ctx.seek_info()["blocks"] == 0
    # without tables the same calls probe whole recipes, and none is served from a table
    big = max(s.ids, key=lambda i: len(lens_of[i]))
    part = [(big, off, 4096, None) for off in range(0, sizes[big] - 4096, sizes[big] // 7)]
    serve(ctx, part, s.blocks, misalign=1)
    info = check_rows(ctx, [q[:3] for q in part], lens_of, sizes, tabled=())
    assert info["last_seek_reqs"] == 0 and info["last_rows"] == len(part) * len(lens_of[big])
    assert ctx.seek_build(s.ids) == [0] * len(s.ids) and ctx.seek_build_code == 0
    info = ctx.seek_info()
    assert info["blocks"] == len(s.ids) and info["chunks"] == sum(map(len, lens_of.values())) and info["bytes"] > 0
    # with them: in proportion to the range
    serve(ctx, part, s.blocks, misalign=1)
    info = check_rows(ctx, [q[:3] for q in part], lens_of, sizes, tabled=set(s.ids))
    if kind == "main":
        assert info["last_rows"] < len(part) * len(lens_of[big]) // 4
    for bid in s.ids:
        reqs = [(bid, off, length, None) for off, length in ranges_of(s, bid)]
        for m in MISALIGN:
            res, _ = serve(ctx, reqs, s.blocks, misalign=m)
            assert ctx.read_batch_code == 0
            check_rows(ctx, [q[:3] for q in reqs], lens_of, sizes, tabled=set(s.ids))
        size = sizes[bid]
        assert res[0] == size and res[2] == 0 and res[3] == 0
        assert np.array_equal(ctx.read_range(bid, 0, size), s.blocks[bid])
        assert ctx.seek_info()["last_seek_reqs"] == 1
        if size >= 3:
            assert np.array_equal(ctx.read_range(bid, size - 3, 100), s.blocks[bid][-3:])
            assert np.array_equal(ctx.read_range(bid, size - 3, 100, verify=True), s.blocks[bid][-3:])
        assert ctx.read_range(bid, size, 5).size == 0
        assert ctx.seek_info()["last_rows"] == 0                               # a zero-length request: no lookup
        with pytest.raises(HdrfError) as e:
            ctx.read_range(bid, size + 1, 1)
        assert e.value.code == INVAL
    # building again rebuilds; dropping some leaves the others
    assert ctx.seek_build(s.ids[:2]) == [0, 0] and ctx.seek_info()["blocks"] == len(s.ids)
    ctx.seek_drop(s.ids[:1] + [123456])
    assert ctx.seek_info()["blocks"] == len(s.ids) - 1
    serve(ctx, [(s.ids[0], 1, 10, None), (s.ids[1], 1, 10, None)], s.blocks)
    assert ctx.seek_info()["last_seek_reqs"] == 1
    ctx.seek_drop(None)
    assert ctx.seek_info()["bytes"] == 0


@gpu
@pytest.mark.parametrize("hasher,compressor", PARAMS)
def test_one_call_mixes_tables_recipes_and_neither(stores, hasher, compressor):
    s = stores("main", hasher, compressor)
    ctx = s.ctx
    ctx.seek_drop(None)
    tabled = set(s.ids[0::2])
    assert ctx.seek_build(sorted(tabled)) == [0] * len(tabled)
    rng = np.random.default_rng(77)
    reqs, kinds = [], []
    while len(reqs) < READ_MAX_REQS:
        bid = s.ids[int(rng.integers(len(s.ids)))]
        size = len(s.blocks[bid])
        length = [1, 2, 15, 16, 17, 700, 4096, 8191, 8192, 8193, 65536, 300_000, size, 0][len(reqs) % 14]
        off = int(rng.integers(0, size + 1))
        if len(reqs) % 3 == 2:                                                  # the recipe travels with the request
            reqs.append((s.recipes[bid], off, length, s.blocks[bid]))
            kinds.append(0)
        else:
            reqs.append((bid, off, length, None))
            kinds.append(1 if bid in tabled else 0)
    assert sum(kinds) > 20 and sum(1 for q, k in zip(reqs, kinds) if not k and q[3] is None) > 20
    res, together = serve(ctx, reqs, s.blocks, misalign=3)
    info = ctx.seek_info()
    assert ctx.read_batch_code == 0 and min(res) >= 0 and info["last_seek_reqs"] == sum(kinds)
    # the same requests, each served alone into the same place of a second buffer
    pos, cursor = [], GUARD
    for _, off, length, _ in reqs:
        pos.append(cursor + 3)
        cursor = (cursor + 3 + length + GUARD + 63) & ~63
    total = cursor + GUARD
    dev = ctx.dev_alloc(total)
    try:
        ctx.h2d(dev, np.full(total, FILL, np.uint8))
        for (blk, off, length, _), p, r, k in zip(reqs, pos, res, kinds):
            assert ctx.read_batch([(blk, off, length, dev + p)], verify=True) == [r]
            assert ctx.read_batch_bad == [-1] and ctx.seek_info()["last_seek_reqs"] == k
        assert np.array_equal(ctx.d2h(dev, total), together)
    finally:
        ctx.dev_free(dev)
        ctx.seek_drop(None)


def tiny_store(hasher):
    """Two raw containers and two recipes with chunks of 0, 1 and many bytes: (files, index rows, recipes,
    blocks, lens); a zero-length chunk is the one entry of the empty digest, named wherever it stands."""
    rng = np.random.default_rng(5)
    files = {7: rng.integers(0, 256, 9000, dtype=np.uint8).tobytes(), 8: rng.integers(0, 256, 9000, dtype=np.uint8).tobytes()}
    lens = {30: [0, 1, 1, 0, 0, 702, 1, 0, 5000, 1, 0, 0], 31: [1, 1, 702, 1, 5000, 1], 32: [0, 0], 33: [9]}
    rows, recipes, blocks, cur = {}, {}, {}, {7: 0, 8: 0}
    for bid, ls in lens.items():
        digs, data = [], b""
        for k, n in enumerate(ls):
            cid = 7 + (k + bid) % 2
            piece = files[cid][cur[cid]:cur[cid] + n]
            d = HASH[hasher](piece).digest()
            rows.setdefault(d, (1, cid, cur[cid], cur[cid] + n))
            cur[cid] += n
            digs.append(d)
            data += piece
        recipes[bid] = len(data).to_bytes(4, "big") + b"".join(digs)
        blocks[bid] = np.frombuffer(data, np.uint8)
    return files, rows, recipes, blocks, lens


@gpu
@pytest.mark.parametrize("hasher", [0, 1])
def test_tiny_and_empty_chunks(hasher):
    files, rows, recipes, blocks, lens = tiny_store(hasher)
    with Context(hasher=hasher, **SMALL) as ctx:
        ctx.index_load(np.frombuffer(b"".join(rows), np.uint8),
                       np.frombuffer(b"".join(enc_value(*v) for v in rows.values()), np.uint8))
        for bid, r in recipes.items():
            ctx.recipe_load(bid, r)
        for cid, data in files.items():
            ctx.container_load(cid, data, lz4=False)
        sizes = {b: len(blocks[b]) for b in blocks}
        for tabled in (False, True):
            if tabled:
                assert ctx.seek_build(list(lens)) == [0] * len(lens)
                assert ctx.seek_info()["blocks"] == 4 and ctx.seek_info()["chunks"] == sum(map(len, lens.values()))
            for bid in lens:
                seams = sorted({0, sizes[bid]} | {int(e) + d for e in np.cumsum(lens[bid]) for d in (-1, 0, 1)
                                                  if 0 <= int(e) + d <= sizes[bid]})
                reqs = [(bid, a, b - a, None) for a in seams for b in seams if b >= a] + [(bid, sizes[bid], 3, None)]
                for at in range(0, len(reqs), READ_MAX_REQS):
                    part = reqs[at:at + READ_MAX_REQS]
                    serve(ctx, part, blocks, misalign=(1, 15)[tabled])
                    assert ctx.read_batch_code == 0
                    check_rows(ctx, [q[:3] for q in part], lens, sizes, tabled=set(lens) if tabled else ())
                    # verified: every chunk under every range hashes to its digest
                    dev = ctx.dev_alloc(64 + sum(q[2] + 1 for q in part))
                    try:
                        at_, vq = 0, []
                        for b_, off, length, _ in part:
                            vq.append((b_, off, length, dev + at_))
                            at_ += length + 1
                        res = ctx.read_batch(vq, verify=True)
                        assert res == [clip(sizes[q[0]], q[1], q[2]) for q in part]
                        assert ctx.read_batch_bad == [-1] * len(part)
                    finally:
                        ctx.dev_free(dev)


@gpu
@pytest.mark.parametrize("hasher,compressor", PARAMS)
def test_only_what_the_range_touches(stores, hasher, compressor):
    s = stores("main", hasher, compressor)
    pick = None
    for x in sorted(c for c, (_, closed) in s.files.items() if closed):
        for bid in s.ids:
            rows = [r for r in s.chunks[bid] if r[2]]
            if any(r[0] == x for r in rows) and any(r[0] != x for r in rows):
                pick = (x, bid)
                break
        if pick:
            break
    assert pick, "no closed container that a block uses only in part"
    x, bid = pick
    rows = [r for r in s.chunks[bid] if r[2]]
    hit = next(r for r in rows if r[0] == x)
    k0 = next(k for k, r in enumerate(rows) if r[0] != x)
    k1 = k0
    while k1 + 1 < len(rows) and rows[k1 + 1][0] != x:
        k1 += 1
    away = (rows[k0][1], rows[k1][1] + rows[k1][2] - rows[k0][1])
    ctx2 = s.restarted(leave_out=set(s.files))                                  # no container is readable
    try:
        assert ctx2.seek_build(s.ids) == [0] * len(s.ids)                       # the build needs only the index
        for cid in s.files:
            if cid != x:
                s.load_container(ctx2, cid)
        reqs = [(bid, away[0], away[1], None), (bid, hit[1], hit[2], None),
                (bid, max(0, hit[1] - 1), 2, None) if hit[1] else (bid, hit[1] + hit[2] - 1, 2, None),
                (bid, 0, len(s.blocks[bid]), None), (bid, away[0], 0, None)]
        res, _ = serve(ctx2, reqs, s.blocks, misalign=15, expect_codes=[0, NOTFOUND, NOTFOUND, NOTFOUND, 0])
        assert res[0] == away[1] > 0 and ctx2.read_batch_code == NOTFOUND and ctx2.seek_info()["last_seek_reqs"] == 5
        with pytest.raises(HdrfError) as e:
            ctx2.read_range(bid, hit[1], hit[2])
        assert e.value.code == NOTFOUND
        s.load_container(ctx2, x)
        whole = [(i, 0, len(s.blocks[i]), None) for i in s.ids]
        res, _ = serve(ctx2, whole, s.blocks)
        assert ctx2.read_batch_code == 0 and ctx2.seek_info()["last_seek_reqs"] == len(s.ids)
    finally:
        ctx2.close()


@gpu
@pytest.mark.parametrize("hasher", [0, 1])
def test_build_failures_are_per_id(hasher):
    with Context(hasher=hasher, **SMALL) as ctx:
        rows, recipes = build(ctx, hasher)
        files = hand_store(hasher)[0]
        ghost = HASH[hasher](b"ghost").digest()
        size = sum(rows[i][4] - rows[i][3] for i in (7, 8))
        ctx.recipe_load(20, size.to_bytes(4, "big") + rows[7][0] + ghost + rows[8][0])
        assert ctx.seek_build([10, 999, 20]) == [0, NOTFOUND, NOTFOUND] and ctx.seek_build_code == NOTFOUND
        assert "block 999" in ctx.L.hdrf_last_error(ctx._h).decode()
        info = ctx.seek_info()
        assert info["blocks"] == 1 and info["chunks"] == len(recipes[10])
        blk = np.frombuffer(b"".join(files[rows[i][2]][rows[i][3]:rows[i][4]] for i in recipes[10]), np.uint8)
        serve(ctx, [(10, 12345, 70_000, None)], {10: blk}, misalign=3)
        assert ctx.seek_info()["last_seek_reqs"] == 1
        # a table whose build fails later is dropped: the lengths of this recipe do not add up
        ctx.recipe_load(21, (size + 1).to_bytes(4, "big") + rows[7][0] + rows[8][0])
        assert ctx.seek_build([21, 10]) == [-7, 0] and ctx.seek_info()["blocks"] == 1
        assert ctx.seek_build([]) == [] and ctx.seek_build_code == 0
    with Context(n_ranks=2, rank=0, max_block_bytes=1 << 20, max_batch_blocks=2, index_log2=16, arena_slots=16,
                 container_max=1 << 21) as ctx:
        with pytest.raises(HdrfError) as e:
            ctx.seek_build([1])
        assert e.value.code == UNSUPPORTED


@gpu
def test_a_table_lives_as_long_as_its_recipe():
    hasher = 0
    with Context(hasher=hasher, **SMALL) as ctx:
        rows, recipes = build(ctx, hasher)
        files = hand_store(hasher)[0]
        blocks = {b: np.frombuffer(b"".join(files[rows[i][2]][rows[i][3]:rows[i][4]] for i in idx), np.uint8)
                  for b, idx in recipes.items()}
        ids = sorted(recipes)
        assert ctx.seek_build(ids) == [0] * len(ids)

        def exact(live):
            reqs = []
            for b in live:
                n = len(blocks[b])
                reqs += [(b, 0, n, None), (b, n // 3, 70_001, None), (b, max(0, n - 9), 100, None)]
            serve(ctx, reqs, blocks, misalign=3)
            assert ctx.read_batch_code == 0 and ctx.seek_info()["last_seek_reqs"] == len(reqs)
            assert ctx.seek_info()["blocks"] == len(live)

        exact(ids)
        ctx.block_delete(11)                                                    # another block goes, and its chunks
        st, _ = ctx.gc()
        assert st["dropped"] > 0
        live = [b for b in ids if b != 11]
        exact(live)
        got, _ = ctx.compact(CIDS)                                              # chunks of blocks 10 and 13 move
        assert [r["status"] for r in got].count(0) >= 1 and sum(r["moved_chunks"] for r in got) > 0
        exact(live)
        for log2 in (12, 10):
            ctx.index_resize(log2)
            exact(live)
        ctx.block_delete(10)                                                    # its own block
        live.remove(10)
        assert ctx.seek_info()["blocks"] == len(live)
        with pytest.raises(HdrfError) as e:
            ctx.read_range(10, 0, 10)
        assert e.value.code == NOTFOUND
        # another recipe under the id: reads follow it, without a table
        new = recipes[12][5:40]
        ctx.recipe_load(12, sum(rows[i][4] - rows[i][3] for i in new).to_bytes(4, "big") + b"".join(rows[i][0] for i in new))
        blocks[12] = np.frombuffer(b"".join(files[rows[i][2]][rows[i][3]:rows[i][4]] for i in new), np.uint8)
        live.remove(12)
        assert ctx.seek_info()["blocks"] == len(live)
        serve(ctx, [(12, 0, len(blocks[12]), None), (12, 700, 5000, None)], blocks, misalign=1)
        assert ctx.seek_info()["last_seek_reqs"] == 0
        assert ctx.seek_build([12]) == [0]
        serve(ctx, [(12, 0, len(blocks[12]), None), (12, 700, 5000, None)], blocks, misalign=1)
        assert ctx.seek_info()["last_seek_reqs"] == 2
        assert ctx.seek_info()["bytes"] > 0
        ctx.reset()
        assert ctx.seek_info()["blocks"] == 0 and ctx.seek_info()["chunks"] == 0
        ctx.seek_drop(None)
        assert ctx.seek_info()["bytes"] == 0


def raw_containers(s):
    """The raw bytes of every container of a Store and where each chunk of each block sits:
    ({container: np.uint8 array}, {block: [(container, start, stop)]}), from the index dump and the blocks."""
    H = s.ctx.H
    where = {bytes(k): dec_value(v) for k, v in zip(s.keys, s.vals)}
    top = {}
    for cid, start, stop in where.values():
        top[cid] = max(top.get(cid, 0), stop)
    raw = {cid: np.zeros(n, np.uint8) for cid, n in top.items()}
    spots = {}
    for bid in s.ids:
        r, spots[bid] = s.recipes[bid], []
        for j, (_, pos, n) in enumerate(s.chunks[bid]):
            cid, start, stop = where[r[4 + H * j:4 + H * (j + 1)]]
            raw[cid][start:stop] = s.blocks[bid][pos:pos + n]
            spots[bid].append((cid, start, stop))
    return raw, spots


def read_one(ctx, bid, off, length, verify):
    """One request into a guarded device buffer: (result, bad position, the bytes written, guards intact)."""
    dev = ctx.dev_alloc(length + 2 * GUARD + 3)
    try:
        ctx.h2d(dev, np.full(length + 2 * GUARD + 3, FILL, np.uint8))
        res = ctx.read_batch([(bid, off, length, dev + GUARD + 3)], verify=verify)
        got = ctx.d2h(dev, length + 2 * GUARD + 3)
    finally:
        ctx.dev_free(dev)
    assert (got[:GUARD + 3] == FILL).all() and (got[GUARD + 3 + length:] == FILL).all()
    return res[0], (ctx.read_batch_bad[0] if verify else None), got[GUARD + 3:GUARD + 3 + length]


@gpu
@pytest.mark.parametrize("hasher,compressor", PARAMS)
def test_verified_ranged_reads(stores, hasher, compressor):
    s = stores("main", hasher, compressor)
    raw, spots = raw_containers(s)
    bid = s.ids[0]
    rows, sp = s.chunks[bid], spots[bid]
    assert len(set(sp)) == len(sp) and len(rows) > 40                          # no chunk of the block twice
    k0, k1 = 10, 30                                                            # the range cuts chunks k0 and k1
    assert all(rows[k][2] >= 3 for k in (k0 - 1, k0, k0 + 5, k0 + 9, k1))
    off = rows[k0][1] + rows[k0][2] // 2 + 1
    end = rows[k1][1] + rows[k1][2] // 2
    # a chunk that ends its container, and the block that holds it: the guarded window
    tb, kl = next((b_, k) for b_ in s.ids for k in range(1, len(spots[b_]))
                  if s.chunks[b_][k][2] >= 3 and s.chunks[b_][k - 1][2] >= 1
                  and spots[b_][k][2] == len(raw[spots[b_][k][0]]))
    trows = s.chunks[tb]
    tail_in = (trows[kl - 1][1], trows[kl - 1][2] + trows[kl][2])              # chunk kl whole: hashed from the output
    tail_cut = (trows[kl][1] + 1, trows[kl][2] - 1)                            # chunk kl cut: hashed from the container
    ctx = s.restarted()
    try:
        def load(b_, flips):
            """Load the containers of block b_'s flipped (chunk, byte-in-chunk) pairs tampered; returns the block as
            it now reads, and a function that restores the clean containers."""
            blk, touched = s.blocks[b_].copy(), {}
            for k, at in flips:
                cid, start, _ = spots[b_][k]
                touched.setdefault(cid, raw[cid].copy())[start + at] ^= 0x40
                blk[s.chunks[b_][k][1] + at] ^= 0x40
            for cid, data in touched.items():
                ctx.container_load(cid, data, lz4=False)
            return blk, lambda: [ctx.container_load(cid, raw[cid], lz4=False) for cid in touched]

        cases = [
            ("inside", bid, (off, end - off), [(k0 + 5, 1)], k0 + 5),
            ("edge, outside the range", bid, (off, end - off), [(k0, 0)], k0),
            ("edge, behind the range", bid, (off, end - off), [(k1, rows[k1][2] - 1)], k1),
            ("before the span", bid, (off, end - off), [(k0 - 1, rows[k0 - 1][2] - 1)], -1),
            ("two", bid, (off, end - off), [(k0 + 9, 2), (k0 + 5, 0), (k1, rows[k1][2] - 1)], k0 + 5),
            ("clean", bid, (off, end - off), [], -1),
            ("tail inside, clean", tb, tail_in, [], -1),
            ("tail cut, clean", tb, tail_cut, [], -1),
            ("tail inside", tb, tail_in, [(kl, trows[kl][2] - 1)], kl),
            ("tail cut", tb, tail_cut, [(kl, 0)], kl),
        ]
        for tabled in (False, True):
            if tabled:
                assert ctx.seek_build(s.ids) == [0] * len(s.ids)
            for name, bid, (o, n), flips, bad in cases:
                blk, restore = load(bid, flips)
                try:
                    r, b, got = read_one(ctx, bid, o, n, verify=True)
                    assert (r, b) == ((CORRUPT, bad) if bad >= 0 else (n, -1)), (name, tabled, r, b)
                    assert np.array_equal(got, blk[o:o + n]), (name, tabled)   # the (tampered) bytes are there anyway
                    assert ctx.seek_info()["last_seek_reqs"] == int(tabled)
                    if bad >= 0:
                        msg = ctx.L.hdrf_last_error(ctx._h).decode()
                        dig = s.recipes[bid][4 + ctx.H * bad:4 + ctx.H * (bad + 1)].hex()
                        assert f"recipe position {bad}" in msg and dig in msg and f"container {spots[bid][bad][0]}" in msg, msg
                        with pytest.raises(HdrfError) as e:
                            ctx.read_range(bid, o, n, verify=True)
                        assert e.value.code == CORRUPT and e.value.bad_chunk == bad
                        assert np.array_equal(e.value.data, blk[o:o + n])
                    else:
                        assert np.array_equal(ctx.read_range(bid, o, n, verify=True), blk[o:o + n])
                    r, _, got = read_one(ctx, bid, o, n, verify=False)          # unverified: returns normally
                    assert r == n and np.array_equal(got, blk[o:o + n]), (name, tabled)
                finally:
                    restore()
        # a batch: only the requests over a bad chunk fail, each with its own position
        bid = s.ids[0]
        flipped, touched = set(), {}
        for b_, k, at in [(bid, k0 + 5, 1), (tb, kl, 0)]:
            cid, start, _ = spots[b_][k]
            touched.setdefault(cid, raw[cid].copy())[start + at] ^= 0x40
            flipped.add(spots[b_][k])
        for cid, data in touched.items():
            ctx.container_load(cid, data, lz4=False)

        def lowest_bad(b_, o, n):
            ks = [k for k, (_, p, ln) in enumerate(s.chunks[b_]) if spots[b_][k] in flipped and p < o + n and p + ln > o]
            return min(ks) if ks else -1

        other = next(i for i in s.ids if i not in (bid, tb) and len(s.blocks[i]) > 80_000)
        reqs = [(bid, off, end - off), (bid, 0, rows[k0][1]), (tb, tail_cut[0], tail_cut[1]), (other, 5, 70_000),
                (bid, rows[k0 + 5][1] + 1, 1)]
        want = [lowest_bad(*q) for q in reqs]
        assert want[0] == k0 + 5 and want[2] == kl and want[4] == k0 + 5 and -1 in want
        assert all(n <= 1 << 20 for _, _, n in reqs)
        dev = ctx.dev_alloc(len(reqs) << 20)                                    # one MiB of output per request
        try:
            res = ctx.read_batch([(s.recipes[b_] if i == 2 else b_, o, n, dev + (i << 20))
                                  for i, (b_, o, n) in enumerate(reqs)], verify=True)
            assert res == [CORRUPT if w >= 0 else q[2] for q, w in zip(reqs, want)] and ctx.read_batch_code == CORRUPT
            assert ctx.read_batch_bad == want
            assert "read request 0" in ctx.L.hdrf_last_error(ctx._h).decode()
            assert ctx.L.hdrf_read_batch_verified(ctx._h, 1, (ReadReq * 1)(), None) == INVAL
        finally:
            ctx.dev_free(dev)
    finally:
        ctx.close()
