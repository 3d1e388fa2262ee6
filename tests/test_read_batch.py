"""Batched, ranged block reads (hdrf_read_batch / hdrf_read_range): many byte ranges of stored blocks
served by one set of launches.  The expected bytes of every read are the slice
block[offset:offset + result] of the numpy array that was written; no oracle is involved."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from helpers import make_block
from hdrf_amd.lib import READ_MAX_REQS, Context, HdrfError, ReadReq, load

gpu = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = 0xA5
GUARD = 64
MISALIGN = (0, 1, 3, 15)
NOTFOUND, INVAL, CAPACITY, UNSUPPORTED = -5, -1, -4, -6
KW = dict(container_max=1 << 20, max_block_bytes=16 << 20, max_batch_blocks=8, index_log2=20, arena_slots=64,
          keep_recipes=1)


# ---- CPU: the ABI and the host-side plan -------------------------------------------------------
def test_null_arguments_are_invalid():
    L = load()
    one = (ReadReq * 1)()
    assert L.hdrf_read_batch(None, 0, None) == INVAL
    assert L.hdrf_read_batch(None, 1, one) == INVAL
    assert L.hdrf_read_range(None, 1, 0, 10, None, 0) == INVAL


def test_read_req_size_matches_the_c_static_assert():
    assert ctypes.sizeof(ReadReq) == 56
    src = open(os.path.join(ROOT, "hdrf_amd", "csrc", "api_views.hip")).read()
    assert "static_assert(sizeof(hdrf_read_req) == 56" in src
    hdr = open(os.path.join(ROOT, "include", "hdrf.h")).read()
    assert "#define HDRF_READ_MAX_REQS %d" % READ_MAX_REQS in hdr


def test_read_plan_under_asan_and_ubsan(tmp_path):
    """tests/cpp/read_plan_test.cpp: clipping and the tile partition against per-byte models, as a
    plain program built with -fsanitize=address,undefined."""
    exe = str(tmp_path / "read_plan_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "read_plan_test.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "PASS" in r.stdout


# ---- the stores --------------------------------------------------------------------------------
def dec_value(v):
    """(container, start, stop) of an 11-byte index value (chunkMeta.getMeta)."""
    v = [int(x) for x in v]
    cid = (v[1] << 16) | (v[2] << 8) | v[3]
    start = ((v[10] & 0xF0) << 20) | (v[4] << 16) | (v[5] << 8) | v[6]
    stop = ((v[10] & 0x0F) << 24) | (v[7] << 16) | (v[8] << 8) | v[9]
    return cid, start, stop


def store_blocks():
    rnd = make_block("random", 11, 1 << 20)
    dup = np.concatenate([rnd[:1 << 19], make_block("random", 12, 1 << 19)])   # chunks in another block's containers
    return [rnd, make_block("text", 13, (1 << 20) + 13), make_block("sparse", 14, 1 << 20), dup,
            make_block("random", 15, 500),                                     # one chunk
            make_block("binary", 16, (1 << 20) + 5), make_block("random", 17, 1 << 20),   # enough bytes to close containers
            np.zeros(0, np.uint8)]                                             # the empty block


def forced_cut_blocks():
    """Bytes >= 0x80 never cut: chunks of 864 / 1,000,001 / 1,299,135 B (the last detected cut is dropped)."""
    return [make_block("random", 7, 2_300_000) | 0x80, make_block("random", 18, 700_000)]


class Store:
    """Blocks reduced into a live context, with what a restart needs and where every chunk lives."""

    def __init__(self, hasher, compressor, blocks, first_id, **over):
        self.hasher, self.compressor = hasher, compressor
        self.kw = dict(KW, hasher=hasher, compressor=compressor, **over)
        self.ctx = Context(**self.kw)
        self.blocks, self.ids, self.ends = {}, [], {}
        for i, b in enumerate(blocks):
            bid = first_id + i
            try:
                res = self.ctx.reduce_block(b, bid)
            except HdrfError:
                if len(b):
                    raise
                continue                                                       # reduce_block refuses length 0
            self.ids.append(bid)
            self.blocks[bid] = b
            self.ends[bid] = [int(x) for x in res["offsets"]]
        ctx = self.ctx
        self.keys, self.vals = ctx.index_dump()
        self.recipes = {i: ctx.recipe(i) for i in self.ids}
        alloc = ctx.allocator()
        self.files = {}
        for t in range(3):
            for cid in range(t << 22, int.from_bytes(alloc[3 * t:3 * t + 3], "big") + 1):
                d, closed = ctx.container(cid)
                if d is not None:
                    self.files[cid] = (d, closed)
        H = ctx.H
        where = {bytes(k): dec_value(v) for k, v in zip(self.keys, self.vals)}
        self.chunks = {}                                                       # id -> [(container, block offset, length)]
        for i in self.ids:
            r, rows, pos = self.recipes[i], [], 0
            for j in range((len(r) - 4) // H):
                cid, start, stop = where[r[4 + H * j:4 + H * (j + 1)]]
                rows.append((cid, pos, stop - start))
                pos += stop - start
            assert pos == len(self.blocks[i]) and [p + n for _, p, n in rows] == self.ends[i]
            self.chunks[i] = rows

    def close(self):
        self.ctx.close()

    def restarted(self, leave_out=(), keep_recipes=1):
        ctx = Context(**dict(self.kw, keep_recipes=keep_recipes))
        ctx.index_load(self.keys, self.vals)
        if keep_recipes:
            for i, r in self.recipes.items():
                ctx.recipe_load(i, r)
        for cid in self.files:
            if cid not in leave_out:
                self.load_container(ctx, cid)
        return ctx

    def load_container(self, ctx, cid):
        d, closed = self.files[cid]
        ctx.container_load(cid, d, closed and self.compressor == 2)


PARAMS = [(0, 1), (1, 2)]
_cache = {}


def _store(kind, hasher, compressor):
    key = (kind, hasher, compressor)
    if key not in _cache:
        if kind == "main":
            s = Store(hasher, compressor, store_blocks(), 5000)
            used = {c for rows in s.chunks.values() for c, _, n in rows if n}
            assert any(closed for _, closed in s.files.values()), "no container closed"
            assert len(used) > 2, "the blocks span no more than two containers"
        else:
            # The write path does not check a chunk's length against container_max, and the 1.3 MB
            # chunk does not fit an arena slot of 1 MiB: this store's containers hold 2 MiB.
            s = Store(hasher, compressor, forced_cut_blocks(), 6000, container_max=1 << 21)
            lens = [n for _, _, n in s.chunks[6000]]
            assert lens == [864, 1_000_001, 1_299_135], lens
        _cache[key] = s
    return _cache[key]


@pytest.fixture(scope="module")
def stores():
    yield _store
    for s in _cache.values():
        s.close()
    _cache.clear()


# ---- helpers -----------------------------------------------------------------------------------
def ranges_of(store, bid):
    """The (offset, length) shapes of the ranges test for one block."""
    size, e = len(store.blocks[bid]), store.ends[bid]
    rows = store.chunks[bid]
    out = [(0, size), (0, 1), (size, 5), (0, 0), (size // 2, 0)]
    if size:
        out += [(size - 1, 1), (size - 3, 100) if size >= 3 else (0, size + 100)]
    inside = next(((p, n) for _, p, n in rows if n >= 3), None)
    if inside:
        out.append((inside[0] + 1, inside[1] - 2))                            # strictly inside one chunk
    if len(e) >= 2:
        k = len(e) // 2 - 1 if len(e) >= 4 else 0
        out += [(e[k], e[k + 1] - e[k]), (e[k] - 1, 2), (e[0] - 1, 2), (e[-2] - 1, 2)]
    if len(e) >= 4:
        for k in sorted({0, min(len(e) // 3, len(e) - 4), len(e) - 4}):
            out.append((e[k] + 1, e[k + 3] - e[k] - 2))
    for k in range(len(rows) - 1):                                             # where the container id changes
        if rows[k][2] and rows[k + 1][2] and rows[k][0] != rows[k + 1][0]:
            seam = rows[k + 1][1]
            out += [(seam - 1, 2), (max(0, seam - 5000), 10_000)]
    rng = np.random.default_rng(bid)
    for j in range(30):
        off = int(rng.integers(0, size + 1))
        cap = 65536 if j % 2 else size + 10
        out.append((off, int(rng.integers(0, cap + 1))))
    return out


def serve(ctx, reqs, blocks, misalign=0, expect_codes=None):
    """reqs: (block id or recipe, offset, length, source block or None).  One read_batch call into one
    device buffer pre-filled with 0xA5, each output `misalign` bytes past a 64-B boundary with at least
    64 guard bytes on both sides.  The whole buffer must equal 0xA5 everywhere but the expected slices.
    Returns (results, the buffer)."""
    pos, cursor = [], GUARD
    for _, off, length, _ in reqs:
        pos.append(cursor + misalign)
        cursor = (cursor + misalign + length + GUARD + 63) & ~63
    total = cursor + GUARD
    want = np.full(total, FILL, np.uint8)
    dev = ctx.dev_alloc(total)
    try:
        ctx.h2d(dev, want)
        res = ctx.read_batch([(blk, off, length, dev + p) for (blk, off, length, _), p in zip(reqs, pos)])
        got = ctx.d2h(dev, total)
    finally:
        ctx.dev_free(dev)
    for i, ((blk, off, length, src), p, r) in enumerate(zip(reqs, pos, res)):
        if expect_codes is not None and expect_codes[i] < 0:
            assert r == expect_codes[i], f"request {i}: {r}"
            continue
        data = blocks[blk] if src is None else src
        n = max(0, min(length, len(data) - off))
        assert r == n, f"request {i} ({off}, {length}) of {len(data)}: result {r}"
        want[p:p + n] = data[off:off + n]
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{bad.size} bytes differ, first at buffer offset {bad[0]} (outputs at {pos[:8]}...)"
    return res, got


# ---- GPU ---------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("hasher,compressor", PARAMS)
@pytest.mark.parametrize("kind", ["main", "forced-cut"])
def test_ranges_equal_slices(stores, kind, hasher, compressor):
    s = stores(kind, hasher, compressor)
    for bid in s.ids:
        reqs = [(bid, off, length, None) for off, length in ranges_of(s, bid)]
        for m in MISALIGN:
            res, _ = serve(s.ctx, reqs, s.blocks, misalign=m)
            assert s.ctx.read_batch_code == 0
        size = len(s.blocks[bid])
        assert res[0] == size and res[2] == 0 and res[3] == 0
        assert np.array_equal(s.ctx.read_range(bid, 0, size), s.blocks[bid])
        if size >= 3:
            assert np.array_equal(s.ctx.read_range(bid, size - 3, 100), s.blocks[bid][-3:])
        assert s.ctx.read_range(bid, size, 5).size == 0


@gpu
@pytest.mark.parametrize("hasher,compressor", PARAMS)
def test_one_batch_of_many_requests(stores, hasher, compressor):
    s = stores("main", hasher, compressor)
    ctx = s.ctx
    rng = np.random.default_rng(99)
    reqs = [(bid, 0, len(s.blocks[bid]), None) for bid in s.ids[:3]]            # whole blocks
    while len(reqs) < READ_MAX_REQS:
        bid = s.ids[int(rng.integers(len(s.ids)))]
        size = len(s.blocks[bid])
        length = [1, 2, 15, 16, 17, 700, 4096, 8191, 8192, 8193, 65536, 300_000][len(reqs) % 12]
        reqs.append((bid, int(rng.integers(0, size + 1)), length, None))
    assert len(reqs) == READ_MAX_REQS
    res, together = serve(ctx, reqs, s.blocks, misalign=3)
    assert ctx.read_batch_code == 0 and min(res) >= 0 and max(res) == len(s.blocks[s.ids[1]])
    # the same requests, each served alone into the same place of a second buffer
    pos, cursor = [], GUARD
    for _, off, length, _ in reqs:
        pos.append(cursor + 3)
        cursor = (cursor + 3 + length + GUARD + 63) & ~63
    total = cursor + GUARD
    dev = ctx.dev_alloc(total)
    try:
        ctx.h2d(dev, np.full(total, FILL, np.uint8))
        for (bid, off, length, _), p, r in zip(reqs, pos, res):
            assert ctx.read_batch([(bid, off, length, dev + p)]) == [r]
        alone = ctx.d2h(dev, total)
        assert np.array_equal(alone, together)
        assert ctx.read_batch([]) == [] and ctx.read_batch_code == 0            # n = 0
        with pytest.raises(HdrfError) as e:                                     # n = HDRF_READ_MAX_REQS + 1
            ctx.read_batch([(s.ids[0], 0, 1, dev + GUARD)] * (READ_MAX_REQS + 1))
        assert e.value.code == INVAL
        assert ctx.L.hdrf_read_batch(ctx._h, 1, None) == INVAL                  # NULL req
        assert np.array_equal(ctx.d2h(dev, total), alone)                       # call-level failures touch no output
    finally:
        ctx.dev_free(dev)


@gpu
@pytest.mark.parametrize("hasher,compressor", PARAMS)
def test_failures_are_per_request(stores, hasher, compressor):
    s = stores("main", hasher, compressor)
    a, b = s.ids[0], s.ids[1]
    reqs = [(a, 1000, 200_000, None), (999_999, 0, 100, None), (b, len(s.blocks[b]) + 1, 10, None),
            (b, 5, 300_001, None)]
    res, _ = serve(s.ctx, reqs, s.blocks, misalign=1, expect_codes=[0, NOTFOUND, INVAL, 0])
    assert res == [200_000, NOTFOUND, INVAL, 300_001]
    assert s.ctx.read_batch_code == NOTFOUND                                    # the first failure's code
    assert "request 1" in s.ctx.L.hdrf_last_error(s.ctx._h).decode()
    res, _ = serve(s.ctx, reqs[2:] + reqs[:2], s.blocks, expect_codes=[INVAL, 0, 0, NOTFOUND])
    assert s.ctx.read_batch_code == INVAL


@gpu
@pytest.mark.parametrize("hasher,compressor", PARAMS)
def test_only_the_touched_containers_need_to_be_readable(stores, hasher, compressor):
    s = stores("main", hasher, compressor)
    # a closed container X and a block with chunks both inside and outside it
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
    k0 = next(k for k, r in enumerate(rows) if r[0] != x)                       # the longest run outside X from there
    k1 = k0
    while k1 + 1 < len(rows) and rows[k1 + 1][0] != x:
        k1 += 1
    away = (rows[k0][1], rows[k1][1] + rows[k1][2] - rows[k0][1])
    ctx2 = s.restarted(leave_out={x})
    try:
        reqs = [(bid, away[0], away[1], None),                                  # avoids X: exact
                (bid, hit[1], hit[2], None),                                    # exactly a chunk of X
                (bid, max(0, hit[1] - 1), 2, None) if hit[1] else (bid, hit[1] + hit[2] - 1, 2, None),   # one byte of it
                (bid, 0, len(s.blocks[bid]), None)]                             # the whole block
        res, _ = serve(ctx2, reqs, s.blocks, misalign=15, expect_codes=[0, NOTFOUND, NOTFOUND, NOTFOUND])
        assert res[0] == away[1] > 0 and ctx2.read_batch_code == NOTFOUND
        with pytest.raises(HdrfError) as e:
            ctx2.read_range(bid, hit[1], hit[2])
        assert e.value.code == NOTFOUND
        s.load_container(ctx2, x)
        whole = [(i, 0, len(s.blocks[i]), None) for i in s.ids]
        res, stored = serve(ctx2, whole, s.blocks)
        assert ctx2.read_batch_code == 0 and res == [len(s.blocks[i]) for i in s.ids]
        ctx3 = s.restarted(keep_recipes=0)                                      # recipes travel with the requests
        try:
            byrec = [(s.recipes[i], 0, len(s.blocks[i]), s.blocks[i]) for i in s.ids]
            res3, carried = serve(ctx3, byrec, s.blocks)
            assert res3 == res and np.array_equal(carried, stored)
            mixed = [(s.recipes[bid], away[0] + 1, away[1], s.blocks[bid]), (bid, 0, 10, None)]
            res3, _ = serve(ctx3, mixed, s.blocks, misalign=1, expect_codes=[0, NOTFOUND])
            assert res3[1] == NOTFOUND and ctx3.read_batch_code == NOTFOUND
        finally:
            ctx3.close()
    finally:
        ctx2.close()


@gpu
def test_read_completes_batches_in_flight():
    blocks = [make_block("random", 51, 900_000), make_block("text", 52, 700_001)]
    with Context(hasher=0, **dict(KW, container_max=4 << 20, max_block_bytes=4 << 20)) as ctx:
        ptrs = []
        for b in blocks:
            p = ctx.dev_alloc(len(b) + 64)
            ctx.h2d(p, b)
            ptrs.append(p)
        ctx.submit_batch(ptrs, [len(b) for b in blocks], [len(b) + 64 for b in blocks], [1, 2])
        got = ctx.read_range(2, 123_457, 400_000)                               # no wait_batch: the read completes it
        assert np.array_equal(got, blocks[1][123_457:523_457])
        assert ctx.stats()["blocks"] == 2 and ctx.index_count() > 0
        assert np.array_equal(ctx.read_range(1, 0, 1 << 30), blocks[0])
        for p in ptrs:
            ctx.dev_free(p)


@gpu
def test_other_entry_points(stores, tmp_path):
    with Context(n_ranks=2, rank=0, max_block_bytes=1 << 20, max_batch_blocks=2, index_log2=16, arena_slots=16,
                 container_max=1 << 21) as ctx:
        with pytest.raises(HdrfError) as e:
            ctx.read_batch([(1, 0, 10, 0)])
        assert e.value.code == UNSUPPORTED
        out = np.zeros(16, np.uint8)
        assert ctx.L.hdrf_read_range(ctx._h, 1, 0, 10, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), 16) == UNSUPPORTED
    s = stores("main", 0, 1)
    out = np.full(64, FILL, np.uint8)
    p = out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    assert s.ctx.L.hdrf_read_range(s.ctx._h, s.ids[0], 10, 100, p, 99) == CAPACITY
    assert (out == FILL).all()
    assert s.ctx.L.hdrf_read_range(s.ctx._h, s.ids[0], (1 << 20) - 7, 100, p, 7) == 7   # cap = the clipped length
    assert np.array_equal(out[:7], s.blocks[s.ids[0]][-7:]) and (out[7:] == FILL).all()
    assert s.ctx.L.hdrf_read_range(s.ctx._h, s.ids[0], (1 << 20) + 1, 1, p, 64) == INVAL
    assert s.ctx.L.hdrf_read_range(s.ctx._h, 424242, 0, 1, p, 64) == NOTFOUND
    # include/hdrf_scheme.hpp: HipReductionScheme::read_range (tests/cpp/read_range_scheme_test.cpp)
    import hdrf_amd.lib as lib
    exe = str(tmp_path / "read_range_scheme_test")
    libdir = os.path.dirname(lib.LIB_PATH)
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "read_range_scheme_test.cpp"), "-o", exe, "-L", libdir, "-lhdrf",
                    "-Wl,-rpath," + libdir], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "PASS" in r.stdout


@gpu
@pytest.mark.parametrize("hasher,compressor", PARAMS)
def test_whole_block_reads_are_unchanged_neighbours(stores, hasher, compressor):
    """hdrf_reconstruct_block shares the d_rd scratch with the batched reads: each path must leave it
    usable by the other."""
    s = stores("main", hasher, compressor)
    whole = [(i, 0, len(s.blocks[i]), None) for i in s.ids]
    serve(s.ctx, whole, s.blocks, misalign=1)
    for i in s.ids:
        assert np.array_equal(s.ctx.reconstruct_block(i), s.blocks[i]), f"block {i}"
        serve(s.ctx, [(i, min(7, len(s.blocks[i])), 100_000, None)], s.blocks)
        assert np.array_equal(s.ctx.reconstruct_block(i, verify=True), s.blocks[i]), f"block {i} verified"
    serve(s.ctx, whole, s.blocks, misalign=15)
