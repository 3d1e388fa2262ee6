"""Block deletion (hdrf_block_delete) and index garbage collection (hdrf_gc).  Expected values come
from hashlib and plain Python over the test's own rows and recipes, never from the code under test."""
import ctypes
import hashlib
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from helpers import make_block, prng_bytes
from hdrf_amd.lib import Context, GcContainer, GcStats, HdrfError, load

gpu = pytest.mark.gpu

HASH = {0: hashlib.sha1, 1: hashlib.sha224}
CIDS = [5, 6, (1 << 22) + 2]               # the hand-built store's containers (two storer ranges)
PER = 300                                  # chunks per container: 900 rows in a table of 1024 slots
SMALL = dict(max_block_bytes=1 << 20, max_batch_blocks=2, index_log2=10, arena_slots=8, container_max=1 << 21)


# ---- CPU: the ABI and the host arithmetic --------------------------------------------------------
def test_struct_sizes_match_the_c_static_asserts():
    """sizeof(hdrf_gc_stats) == 80 and sizeof(hdrf_gc_container) == 40 (api_gc.hip)."""
    assert ctypes.sizeof(GcStats) == 80
    assert ctypes.sizeof(GcContainer) == 40
    src = open(os.path.join(ROOT, "hdrf_amd", "csrc", "api_gc.hip")).read()
    assert "static_assert(sizeof(hdrf_gc_stats) == 80" in src
    assert "static_assert(sizeof(hdrf_gc_container) == 40" in src


def test_null_context_is_invalid():
    L = load()
    assert L.hdrf_block_delete(None, 1) == -1
    st = GcStats()
    assert L.hdrf_gc(None, 0, ctypes.byref(st), None, 0) == -1
    assert L.hdrf_gc(None, 1, None, None, 0) == -1


def test_gc_plan_under_asan_and_ubsan(tmp_path):
    """tests/cpp/gc_plan_test.cpp: the flat-range arithmetic of the mark pass against a per-digest
    model, as a plain program built with -fsanitize=address,undefined."""
    exe = str(tmp_path / "gc_plan_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "gc_plan_test.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "PASS" in r.stdout


# ---- the hand-built store and its Python model -----------------------------------------------------
def enc_value(ncopy, cid, start, stop):
    """chunkMeta.getMeta: the 11-byte index value."""
    return bytes([ncopy & 0xFF, (cid >> 16) & 0xFF, (cid >> 8) & 0xFF, cid & 0xFF,
                  (start >> 16) & 0xFF, (start >> 8) & 0xFF, start & 0xFF,
                  (stop >> 16) & 0xFF, (stop >> 8) & 0xFF, stop & 0xFF,
                  ((start >> 20) & 0xF0) | ((stop >> 24) & 0x0F)])


def dec_value(v):
    v = [int(x) for x in v]
    cid = (v[1] << 16) | (v[2] << 8) | v[3]
    start = ((v[10] & 0xF0) << 20) | (v[4] << 16) | (v[5] << 8) | v[6]
    stop = ((v[10] & 0x0F) << 24) | (v[7] << 16) | (v[8] << 8) | v[9]
    return cid, start, stop


_STORES = {}


def hand_store(hasher):
    """(files, rows, recipes): three raw containers carved back to back into 300 chunks each; rows =
    (digest, ncopy, container, start, stop); recipes = {block id: [row index, ...]}: four that overlap
    pairwise and cover every row, one of them with one digest 50 times, and an empty one."""
    if hasher not in _STORES:
        files, rows, x = {}, [], 777
        for c, cid in enumerate(CIDS):
            lens = []
            for _ in range(PER):
                x = (x * 1103515245 + 12345) & 0x7FFFFFFF
                lens.append(40 + (x >> 8) % 1200)
            data = prng_bytes(900 + c, sum(lens)).tobytes()
            pos = 0
            for n in lens:
                rows.append((HASH[hasher](data[pos:pos + n]).digest(), 1 + len(rows) % 3, cid, pos, pos + n))
                pos += n
            files[cid] = data
        assert len({r[0] for r in rows}) == len(rows) == 900
        recipes = {
            10: list(range(0, 400)),
            11: list(range(300, 650)),
            12: list(range(600, 900)) + list(range(0, 50)),
            13: list(range(350, 380)) + [420] * 50 + list(range(640, 660)),
            14: [],
        }
        assert set().union(*map(set, recipes.values())) == set(range(900))
        _STORES[hasher] = (files, rows, recipes)
    return _STORES[hasher]


def recipe_bytes(rows, idx, extra=()):
    """[BE32 size | digests] of the rows idx (+ digests that are in no row)."""
    size = sum(rows[i][4] - rows[i][3] for i in idx)
    return size.to_bytes(4, "big") + b"".join(rows[i][0] for i in idx) + b"".join(extra)


def build(ctx, hasher, load_containers=True):
    files, rows, recipes = hand_store(hasher)
    keys = np.frombuffer(b"".join(r[0] for r in rows), np.uint8)
    vals = np.frombuffer(b"".join(enc_value(*r[1:]) for r in rows), np.uint8)
    ctx.index_load(keys, vals)
    for bid, idx in recipes.items():
        ctx.recipe_load(bid, recipe_bytes(rows, idx))
    if load_containers:
        for cid, data in files.items():
            ctx.container_load(cid, data, lz4=False)
    return rows, dict(recipes)


def model(rows, recipes, readable, extra_digests=0):
    """What hdrf_gc must report for the index `rows` and the live recipes {id: [row index]}."""
    live = set()
    for idx in recipes.values():
        live.update(idx)
    kept = [i for i in range(len(rows)) if i in live]
    dropped = [i for i in range(len(rows)) if i not in live]
    nbytes = lambda ix: sum(rows[i][4] - rows[i][3] for i in ix)
    cont = []
    for cid in sorted({r[2] for r in rows}):
        k = [i for i in kept if rows[i][2] == cid]
        d = [i for i in dropped if rows[i][2] == cid]
        cont.append(dict(id=cid, readable=int(cid in readable), kept_chunks=len(k), kept_bytes=nbytes(k),
                         dropped_chunks=len(d), dropped_bytes=nbytes(d)))
    stats = dict(recipes=len(recipes), recipe_digests=sum(len(v) for v in recipes.values()) + extra_digests,
                 entries=len(rows), kept=len(kept), dropped=len(dropped), kept_bytes=nbytes(kept),
                 dropped_bytes=nbytes(dropped), missing=extra_digests, containers=len(cont),
                 dead_containers=sum(1 for c in cont if c["kept_chunks"] == 0))
    return stats, cont, kept, dropped


def dump_of(rows, idx):
    """The index dump of the rows idx: (keys, values) sorted by digest."""
    srt = sorted((rows[i][0], enc_value(*rows[i][1:])) for i in idx)
    H = len(rows[0][0])
    return (np.frombuffer(b"".join(k for k, _ in srt), np.uint8).reshape(-1, H),
            np.frombuffer(b"".join(v for _, v in srt), np.uint8).reshape(-1, 11))


def same_dump(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def delete_and_collect(ctx, rows, recipes, victim):
    """Delete `victim`, dry run, collect, collect again: every step against the model."""
    before = ctx.index_dump()
    assert same_dump(before, dump_of(rows, range(len(rows))))
    ctx.block_delete(victim)
    del recipes[victim]
    stats, cont, kept, dropped = model(rows, recipes, CIDS)
    assert 0 < len(kept) < len(rows)
    st, got = ctx.gc(dry=True)
    print("dry:", st)
    assert st == stats and got == cont
    after_dry = ctx.index_dump()
    assert after_dry[0].tobytes() == before[0].tobytes() and after_dry[1].tobytes() == before[1].tobytes()
    st, got = ctx.gc()
    assert st == stats and got == cont
    after = ctx.index_dump()
    want = dump_of(rows, kept)
    assert after[0].tobytes() == want[0].tobytes() and after[1].tobytes() == want[1].tobytes()
    assert ctx.index_count() == len(kept)
    for i in dropped:
        assert ctx.index_get(rows[i][0]) is None, f"dropped row {i} is still in the index"
    for i in kept[::37]:
        assert ctx.index_get(rows[i][0]) == enc_value(*rows[i][1:])
    sst, bad = ctx.scrub()
    assert bad == [] and sst["bad"] == 0 and sst["entries"] == sst["checked"] == len(kept)
    stats2, cont2, kept2, dropped2 = model([rows[i] for i in kept], {b: [kept.index(i) for i in v]
                                                                   for b, v in recipes.items()}, CIDS)
    assert dropped2 == []
    st, got = ctx.gc()                                            # a second collection drops nothing
    assert st == stats2 and got == cont2 and st["dropped"] == 0
    assert same_dump(ctx.index_dump(), want)
    return kept


# ---- GPU: the hand-built store ---------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("hasher", [0, 1])
def test_small_full_table(hasher):
    """900 rows in 1024 slots: long probe clusters, some wrapping past the table's end."""
    with Context(hasher=hasher, **SMALL) as ctx:
        rows, recipes = build(ctx, hasher)
        kept = delete_and_collect(ctx, rows, recipes, 11)
        # the blocks that remain still read back from the collected index
        files = hand_store(hasher)[0]
        for bid, idx in recipes.items():
            want = b"".join(files[rows[i][2]][rows[i][3]:rows[i][4]] for i in idx)
            assert ctx.reconstruct_block(bid, verify=True).tobytes() == want
        assert set(kept) == set().union(*map(set, recipes.values()))


@gpu
def test_tag_collisions():
    """The same with 4 tag bits (SHA-1): mark and rebuild go through entries that share a tag."""
    with Context(hasher=0, debug_tag_bits=4, **SMALL) as ctx:
        rows, recipes = build(ctx, 0)
        delete_and_collect(ctx, rows, recipes, 11)


@gpu
@pytest.mark.parametrize("hasher", [0, 1])
def test_nothing_or_everything(hasher):
    """No container is loaded here: every container id is seen only in entries."""
    with Context(hasher=hasher, **SMALL) as ctx:
        rows, recipes = build(ctx, hasher, load_containers=False)
        before = ctx.index_dump()
        stats, cont, kept, dropped = model(rows, recipes, [])
        assert dropped == [] and stats["dead_containers"] == 0
        st, got = ctx.gc()                                        # nothing deleted: nothing changes
        assert st == stats and got == cont
        assert same_dump(ctx.index_dump(), before)
        for bid in list(recipes):
            ctx.block_delete(bid)
        stats, cont, kept, dropped = model(rows, {}, [])
        st, got = ctx.gc()
        assert st == stats and got == cont
        assert st["kept"] == st["kept_bytes"] == 0 and st["dropped"] == len(rows)
        assert st["dead_containers"] == st["containers"] == len(CIDS)
        assert all(c["kept_chunks"] == 0 and c["readable"] == 0 for c in got)
        assert ctx.index_count() == 0
        st, got = ctx.gc()                                        # an empty index has no container rows
        assert got == [] and st["entries"] == st["containers"] == 0


@gpu
@pytest.mark.parametrize("hasher", [0, 1])
def test_recipe_digest_absent_from_the_index(hasher):
    with Context(hasher=hasher, **SMALL) as ctx:
        rows, recipes = build(ctx, hasher)
        ghosts = [HASH[hasher](b"ghost %d" % i).digest() for i in (1, 2, 2)]      # one of them twice
        ctx.recipe_load(20, recipe_bytes(rows, [7, 8], ghosts))
        recipes[20] = [7, 8]
        ctx.block_delete(12)
        del recipes[12]
        stats, cont, kept, dropped = model(rows, recipes, CIDS, extra_digests=3)
        st, got = ctx.gc()
        assert st == stats and got == cont and st["missing"] == 3
        assert same_dump(ctx.index_dump(), dump_of(rows, kept))


@gpu
@pytest.mark.parametrize("hasher", [0, 1])
def test_more_containers_than_the_sweep_keeps_on_chip(hasher):
    """900 containers, one per row: the sweep keeps the first 768 ids and their counters in LDS and
    goes to memory for the rest.  None is loaded, so all of them are learned from the entries."""
    _, rows, recipes = hand_store(hasher)
    rows = [(r[0], r[1], 10 + 3 * i, r[3], r[4]) for i, r in enumerate(rows)]
    with Context(hasher=hasher, **SMALL) as ctx:
        ctx.index_load(np.frombuffer(b"".join(r[0] for r in rows), np.uint8),
                       np.frombuffer(b"".join(enc_value(*r[1:]) for r in rows), np.uint8))
        live = {b: idx for b, idx in recipes.items() if b != 11}
        for bid, idx in live.items():
            ctx.recipe_load(bid, recipe_bytes(rows, idx))
        stats, cont, kept, dropped = model(rows, live, [])
        assert stats["containers"] == 900 and 0 < stats["dead_containers"] < 900
        for dry in (True, False):
            st, got = ctx.gc(dry=dry)
            assert st == stats and got == cont
        assert same_dump(ctx.index_dump(), dump_of(rows, kept))


@gpu
def test_epoch_wrap():
    """254 resets take the table epoch to 255: the rebuild crosses 255 -> 1 through the real clear."""
    with Context(hasher=0, **SMALL) as ctx:
        for _ in range(254):
            ctx.reset()
        rows, recipes = build(ctx, 0)
        ctx.block_delete(10)
        del recipes[10]
        stats, cont, kept, dropped = model(rows, recipes, CIDS)
        st, got = ctx.gc()
        assert st == stats and got == cont
        assert same_dump(ctx.index_dump(), dump_of(rows, kept))
        for i in dropped:
            assert ctx.index_get(rows[i][0]) is None
        sst, bad = ctx.scrub()
        assert bad == [] and sst["entries"] == sst["checked"] == len(kept)
        ctx.block_delete(13)                                      # and once more in the new epoch
        del recipes[13]
        stats, cont, kept2, _ = model([rows[i] for i in kept], {b: [kept.index(i) for i in v]
                                                               for b, v in recipes.items()}, CIDS)
        st, got = ctx.gc()
        assert st == stats and got == cont
        assert same_dump(ctx.index_dump(), dump_of([rows[i] for i in kept], kept2))


@gpu
def test_errors():
    L = load()
    with Context(hasher=0, **SMALL) as ctx:
        rows, recipes = build(ctx, 0)
        with pytest.raises(HdrfError) as e:
            ctx.block_delete(999)
        assert e.value.code == -5
        rx = ctx.rx_begin(50)                                     # a receive is open
        with pytest.raises(HdrfError) as e:
            ctx.gc()
        assert e.value.code == -1
        with pytest.raises(HdrfError) as e:
            ctx.gc(dry=True)
        assert e.value.code == -1
        ctx.rx_cancel(rx)
        assert L.hdrf_gc(ctx._h, 2, None, None, 0) == -1          # an unknown flag
        assert L.hdrf_gc(ctx._h, 0, None, None, 5) == -1          # rows without a buffer
        rb = ctx.stats()["recipe_bytes"]
        assert ctx.block_length(10) == sum(rows[i][4] - rows[i][3] for i in recipes[10])
        ctx.block_delete(10)
        assert ctx.stats()["recipe_bytes"] == max(0, rb - (4 + 20 * len(recipes[10])))
        assert ctx.recipe(10) is None
        out = np.zeros(1 << 20, np.uint8)
        op = out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
        bad = ctypes.c_int64(0)
        assert L.hdrf_block_length(ctx._h, 10) == -5
        assert L.hdrf_reconstruct_block(ctx._h, 10, op, out.size) == -5
        assert L.hdrf_reconstruct_block_verified(ctx._h, 10, op, out.size, ctypes.byref(bad)) == -5
        assert L.hdrf_read_range(ctx._h, 10, 0, 100, op, out.size) == -5
        with pytest.raises(HdrfError) as e:
            ctx.block_delete(10)                                  # twice
        assert e.value.code == -5
        assert ctx.block_length(11) > 0                           # the others are untouched
    with Context(hasher=0, keep_recipes=0, **SMALL) as ctx:
        with pytest.raises(HdrfError) as e:
            ctx.gc()
        assert e.value.code == -1
    with Context(n_ranks=2, rank=0, max_block_bytes=1 << 20, max_batch_blocks=2, index_log2=16, arena_slots=16,
                 container_max=1 << 21) as ctx:
        with pytest.raises(HdrfError) as e:
            ctx.gc()
        assert e.value.code == -6


@gpu
def test_delete_covers_stream_mode_blocks():
    """A stream-mode block has a length and no recipe: the delete drops the length."""
    blk = make_block("text", 5, 100_000)
    with Context(hasher=0, **SMALL) as ctx:
        ctx.stream_block_host(4, 77, blk, [len(blk)])
        assert ctx.block_length(77) == len(blk)
        ctx.block_delete(77)
        with pytest.raises(HdrfError) as e:
            ctx.block_length(77)
        assert e.value.code == -5


# ---- GPU: the real write path ------------------------------------------------------------------------
def write_blocks():
    """Six 1 MiB blocks, about half of each made of segments the others share."""
    shared = [make_block(k, 40 + i, 256 << 10) for i, k in enumerate(["random", "text", "binary", "random"])]
    blocks = []
    for i in range(6):
        parts = [shared[i % 4], make_block("random", 500 + i, 256 << 10), shared[(i + 1) % 4],
                 make_block("text", 600 + i, 256 << 10)]
        blocks.append(np.concatenate(parts))
    return blocks


def snapshot(ctx, ids):
    """The persisted state of a DataNode: index rows, allocator, recipes, container files."""
    keys, vals = ctx.index_dump()
    alloc = ctx.allocator()
    recipes = {i: ctx.recipe(i) for i in ids}
    files = {}
    for t in range(3):
        for cid in range(t << 22, int.from_bytes(alloc[3 * t:3 * t + 3], "big") + 1):
            d, closed = ctx.container(cid)
            if d is not None:
                files[cid] = (d, closed)
    return keys, vals, alloc, recipes, files


@gpu
@pytest.mark.parametrize("hasher,compressor", [(0, 1), (1, 2)])
def test_real_write_path_and_twin(hasher, compressor):
    """A collected DataNode behaves as one that never held the dropped chunks: a twin restored from the
    collected state makes the same decisions, byte for byte."""
    H = HASH[hasher]().digest_size
    kw = dict(hasher=hasher, compressor=compressor, container_max=1 << 20, max_block_bytes=4 << 20,
              max_batch_blocks=2, index_log2=16, arena_slots=32)
    blocks = write_blocks()
    ids = [100 + i for i in range(6)]
    gone = [101, 104]
    left = [i for i in ids if i not in gone]
    with Context(**kw) as a, Context(**kw) as b:
        for blk, i in zip(blocks, ids):
            a.reduce_block(blk, i)
        keys0, vals0, _, recipes0, files0 = snapshot(a, ids)
        assert any(closed for _, closed in files0.values()), "no container closed"
        rb = a.stats()["recipe_bytes"]
        for i in gone:
            a.block_delete(i)
        assert a.stats()["recipe_bytes"] == rb - sum(len(recipes0[i]) for i in gone)
        live = {recipes0[i][4 + H * j:4 + H * (j + 1)] for i in left for j in range((len(recipes0[i]) - 4) // H)}
        keep = [n for n, k in enumerate(keys0) if bytes(k) in live]
        assert 0 < len(keep) < len(keys0)
        st, rows = a.gc()
        print("gc:", st)
        assert (st["entries"], st["kept"], st["dropped"], st["missing"]) == (len(keys0), len(keep), len(keys0) - len(keep), 0)
        assert st["recipes"] == len(left) and st["recipe_digests"] == sum((len(recipes0[i]) - 4) // H for i in left)
        locs = [dec_value(v) for v in vals0]
        assert st["kept_bytes"] == sum(locs[n][2] - locs[n][1] for n in keep)
        assert [r["id"] for r in rows] == sorted({c for c, _, _ in locs})
        for r in rows:
            assert r["kept_chunks"] == sum(1 for n in keep if locs[n][0] == r["id"])
            assert r["readable"] == 1
        keys1, vals1, alloc1, recipes1, files1 = snapshot(a, left)
        assert np.array_equal(keys1, keys0[keep]) and np.array_equal(vals1, vals0[keep])
        assert files1 == files0 and recipes1 == {i: recipes0[i] for i in left}
        for blk, i in zip(blocks, ids):
            if i in left:
                assert np.array_equal(a.reconstruct_block(i, verify=True), blk), f"block {i}"
        dev = a.dev_alloc(1 << 20)                                # ranges that straddle chunks
        spans = [(100, 1000, 300_000), (102, 262_000, 5_000), (103, 0, 1), (105, 700_001, 1 << 20)]
        for bid, off, n in spans:
            want = blocks[bid - 100][off:off + n]
            assert a.read_batch([(bid, off, n, dev)]) == [len(want)]
            assert np.array_equal(a.d2h(dev, len(want)), want)
        assert a.read_batch([(101, 0, 10, dev)]) == [-5]
        a.dev_free(dev)
        # the twin: a fresh DataNode restored from the collected state
        b.index_load(keys1, vals1)
        opens = []
        for t in range(3):
            d = files1.get(int.from_bytes(alloc1[3 * t:3 * t + 3], "big"))
            opens.append(d[0] if d is not None and not d[1] else None)
        b.allocator_load(alloc1, opens)
        for i, r in recipes1.items():
            b.recipe_load(i, r)
        more = [(200, blocks[1]),                                 # the bytes of a deleted block
                (201, np.concatenate([blocks[4][:300_000], make_block("random", 900, 400_000), blocks[0][:200_000]]))]
        for bid, blk in more:
            ra, rb_ = a.reduce_block(blk, bid), b.reduce_block(blk, bid)
            for f in ("offsets", "digests", "is_new", "container_id", "container_pos"):
                assert np.array_equal(ra[f], rb_[f]), f"block {bid}: {f}"
            assert ra["store_size"] == rb_["store_size"]
            ba, bb = a.batch_result(0), b.batch_result(0)
            for f in ("offsets", "digests", "is_new", "container_id", "container_pos"):
                assert np.array_equal(ba[f], bb[f]), f"block {bid}: batch {f}"
            assert ra["is_new"].any() and not ra["is_new"].all()  # some chunks were kept, some dropped or fresh
        ka, va = a.index_dump()
        kb, vb = b.index_dump()
        assert np.array_equal(ka, kb) and np.array_equal(va, vb)
        assert a.allocator() == b.allocator()
        alloc2 = a.allocator()
        seen = 0
        for t in range(3):
            for cid in range(t << 22, int.from_bytes(alloc2[3 * t:3 * t + 3], "big") + 1):
                db, cb = b.container(cid)
                if db is None:                                    # closed before the restart: a file of the first run
                    continue
                assert (db, cb) == a.container(cid), f"container {cid}"
                seen += 1
        assert seen >= 3
        for cid, (d, closed) in files1.items():                   # the twin reads everything back too
            if b.container(cid)[0] is None:
                b.container_load(cid, d, closed and compressor == 2)
        for bid, blk in [(i, blocks[i - 100]) for i in left] + more:
            assert np.array_equal(b.reconstruct_block(bid, verify=True), blk), f"twin block {bid}"
            assert np.array_equal(a.reconstruct_block(bid, verify=True), blk), f"block {bid}"
