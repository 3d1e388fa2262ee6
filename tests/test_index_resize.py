"""The fingerprint table's size, online (hdrf_index_info_get, hdrf_index_resize).  Expected values come
from hashlib, plain Python over the test's own rows, and the oracle, never from the code under test.
The hand-built store is tests/test_gc.py's: 900 unique rows, three containers, five recipes, in a
1024-slot table whose probe clusters wrap past the end."""
import ctypes
import hashlib
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from helpers import compare_block, compare_state, make_block
from hdrf_amd.lib import Context, HdrfError, IndexInfo, load
from hdrf_amd.scheme import HipReductionScheme
from test_boundary import _apply
from test_gc import SMALL, build, delete_and_collect, dump_of, enc_value, hand_store, same_dump

gpu = pytest.mark.gpu


# ---- CPU: the ABI and the host arithmetic --------------------------------------------------------
def test_struct_size_matches_the_c_static_assert():
    assert ctypes.sizeof(IndexInfo) == 32
    src = open(os.path.join(ROOT, "hdrf_amd", "csrc", "api_resize.hip")).read()
    assert "static_assert(sizeof(hdrf_index_info) == 32" in src


def test_null_context_is_invalid():
    L = load()
    info = IndexInfo()
    assert L.hdrf_index_info_get(None, ctypes.byref(info)) == -1
    assert L.hdrf_index_resize(None, 12) == -1


def test_resize_plan_under_asan_and_ubsan(tmp_path):
    """tests/cpp/resize_plan_test.cpp: the argument and load rule at their edges and
    tag_home(t, k + d) >> d == tag_home(t, k), as a plain program built with -fsanitize=address,undefined."""
    exe = str(tmp_path / "resize_plan_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "resize_plan_test.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "PASS" in r.stdout


# ---- helpers ---------------------------------------------------------------------------------------
def info_of(log2, entries):
    return dict(index_log2=log2, slots=1 << log2, entries=entries, table_bytes=64 << log2)


def load_rows(ctx, rows):
    ctx.index_load(np.frombuffer(b"".join(r[0] for r in rows), np.uint8),
                   np.frombuffer(b"".join(enc_value(*r[1:]) for r in rows), np.uint8))


def all_rows_found(ctx, rows):
    for r in rows:
        assert ctx.index_get(r[0]) == enc_value(*r[1:])


def refused(code, call, *a):
    with pytest.raises(HdrfError) as e:
        call(*a)
    assert e.value.code == code, e.value


def one_more_block(ctx, hasher, seed):
    """A context that refused a resize still writes: one block, oracle-exact (the loaded rows name other
    digests and the allocator is a fresh DataNode's, so a fresh oracle is the reference)."""
    from oracle.oracle import Oracle
    blk = make_block("random", seed, 200_000)
    compare_block(ctx.reduce_block(blk, 77), Oracle(hasher=hasher, max_size=SMALL["container_max"]).reduce(blk, 77),
                  tag="after a refusal")


def moved_store_is_whole(ctx, hasher, rows, recipes, log2):
    """The hand-built store after a resize: same dump, every row, every block, a clean scrub."""
    files = hand_store(hasher)[0]
    assert same_dump(ctx.index_dump(), dump_of(rows, range(len(rows))))
    assert ctx.index_count() == len(rows)
    assert ctx.index_info() == info_of(log2, len(rows))
    all_rows_found(ctx, rows)
    for bid, idx in recipes.items():
        want = b"".join(files[rows[i][2]][rows[i][3]:rows[i][4]] for i in idx)
        assert ctx.reconstruct_block(bid, verify=True).tobytes() == want
    sst, bad = ctx.scrub()
    assert bad == [] and sst["bad"] == 0 and sst["entries"] == sst["checked"] == len(rows)


# ---- GPU: the hand-built store ---------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("hasher", [0, 1])
@pytest.mark.parametrize("new_log2", [11, 14])
def test_grow_hand_built_store(hasher, new_log2):
    """1. 900 rows in 2^10 slots moved into 2^11 and (more than one bit) 2^14: nothing but the slots
    changes, and the moved entries are ordinary entries to a delete + collection afterwards."""
    with Context(hasher=hasher, **SMALL) as ctx:
        rows, recipes = build(ctx, hasher)
        before = ctx.index_dump()
        assert same_dump(before, dump_of(rows, range(900))) and ctx.index_count() == 900
        assert ctx.index_info() == info_of(10, 900)
        ctx.index_resize(new_log2)
        after = ctx.index_dump()
        assert after[0].tobytes() == before[0].tobytes() and after[1].tobytes() == before[1].tobytes()
        moved_store_is_whole(ctx, hasher, rows, recipes, new_log2)
        delete_and_collect(ctx, rows, recipes, 11)
        assert ctx.index_info()["index_log2"] == new_log2


@gpu
def test_tag_collisions():
    """2. The same with 4 tag bits (SHA-1), 10 -> 11 -> 10: entries that share a tag each get a slot of
    their own and are still told apart.  The shrink is refused: 900 > 768."""
    with Context(hasher=0, debug_tag_bits=4, **SMALL) as ctx:
        rows, recipes = build(ctx, 0)
        ctx.index_resize(11)
        moved_store_is_whole(ctx, 0, rows, recipes, 11)
        refused(-4, ctx.index_resize, 10)
        moved_store_is_whole(ctx, 0, rows, recipes, 11)
        delete_and_collect(ctx, rows, recipes, 11)


@gpu
@pytest.mark.parametrize("hasher", [0, 1])
def test_shrink_and_the_load_rule(hasher):
    """3. 768 rows fit 2^10 slots (75 %), 769 do not; refusals change nothing and the context goes on."""
    rows = hand_store(hasher)[1]
    big = dict(SMALL, index_log2=14)
    with Context(hasher=hasher, **big) as ctx:
        load_rows(ctx, rows[:768])
        ctx.index_resize(10)
        assert ctx.index_info() == info_of(10, 768)
        assert same_dump(ctx.index_dump(), dump_of(rows, range(768)))
        all_rows_found(ctx, rows[:768])
        assert ctx.index_get(rows[768][0]) is None
    with Context(hasher=hasher, **big) as ctx:
        load_rows(ctx, rows[:769])
        want = dump_of(rows, range(769))
        for code, log2 in [(-4, 10), (-1, 9), (-1, 32), (-1, -1)]:
            refused(code, ctx.index_resize, log2)
            assert ctx.index_info() == info_of(14, 769) and same_dump(ctx.index_dump(), want)
        ctx.index_resize(14)                                      # the current size: 0, nothing happens
        assert ctx.index_info() == info_of(14, 769) and same_dump(ctx.index_dump(), want)
        one_more_block(ctx, hasher, 31)
        all_rows_found(ctx, rows[:769:13])
        ctx.index_resize(11)                                      # 769 of 2048: allowed
        assert ctx.index_info()["index_log2"] == 11 and ctx.index_info()["entries"] == ctx.index_count() > 769
        all_rows_found(ctx, rows[:769])


# ---- GPU: the real write path ------------------------------------------------------------------------
@gpu
def test_a_node_that_outgrows_its_table():
    """4. The headline case.  Two 1 MiB random blocks put 2,198 entries into 2^12 slots (over 50 %); the
    scheme grows the table to 2^13 and goes on: a repeat of block 1 finds every moved entry, a half
    fresh / half old block and a fresh block store only their fresh chunks, all oracle-exact.  The fresh
    bytes are text, which cuts finer (about 1,410 chunks per MiB): the five blocks hold 4,312 distinct
    chunks (the oracle's count, asserted below to be more than 2^12), more than the slots the context
    opened with, so they could not have been stored without the resize."""
    from oracle.oracle import Oracle
    s = HipReductionScheme(index_log2=12, max_block_bytes=1 << 20, max_batch_blocks=1, arena_slots=8)
    ora = Oracle()
    b1, b2 = make_block("random", 1201, 1 << 20), make_block("random", 1202, 1 << 20)
    blocks = [b1, b2, b1.copy(),
              np.concatenate([make_block("text", 1203, 1 << 19), b2[:1 << 19]]), make_block("text", 1204, 1 << 20)]
    ids = [9000 + i for i in range(5)]
    try:
        for i in (0, 1):
            compare_block(s.reduce(blocks[i], ids[i]), ora.reduce(blocks[i], ids[i]), tag=f"block {i}")
        info = s.index_info()
        assert info["index_log2"] == 12 and 2 * info["entries"] > info["slots"]
        assert s.grow_index_if_loaded(0.99) is None and s.index_info() == info
        assert s.grow_index_if_loaded(0.5) == 13
        assert s.index_info() == info_of(13, info["entries"])
        for i in (2, 3, 4):
            got = s.reduce(blocks[i], ids[i])
            compare_block(got, ora.reduce(blocks[i], ids[i]), tag=f"block {i}")
            if i == 2:
                assert len(got["is_new"]) > 1000 and not got["is_new"].any(), "a moved entry was not found"
            else:
                assert got["is_new"].any()
        compare_state(s.ctx, ora, ids, tag="outgrown")
        assert len(ora.index_dump()[0]) > 1 << 12
        assert s.index_info()["entries"] == len(ora.index_dump()[0])
        assert s.grow_index_if_loaded() is None                   # 4,400 of 8,192: under 60 %
        for i in ids:
            assert s.reconstruct(i, verify=True) == blocks[i - 9000].tobytes()
    finally:
        s.close()


_MANY = {}


def many_rows():
    """250,000 rows from hashlib over a counter; the values encode the counter."""
    if not _MANY:
        n = 250_000
        digs = [hashlib.sha1(b"resize row %d" % i).digest() for i in range(n)]
        vals = [enc_value(1 + i % 3, i >> 8, (i & 255) * 1000, (i & 255) * 1000 + 1 + i % 997) for i in range(n)]
        order = sorted(range(n), key=digs.__getitem__)
        _MANY["load"] = (np.frombuffer(b"".join(digs), np.uint8), np.frombuffer(b"".join(vals), np.uint8))
        _MANY["dump"] = (np.frombuffer(b"".join(digs[i] for i in order), np.uint8).reshape(n, 20),
                         np.frombuffer(b"".join(vals[i] for i in order), np.uint8).reshape(n, 11))
    return _MANY["load"], _MANY["dump"]


@gpu
def test_many_tiles_per_workgroup():
    """5. The walk launches min(4 x CUs, tiles) workgroups, 1,024 on a 256-CU part: 2^19 slots (2,048
    tiles) is the smallest table where a workgroup takes a second tile.  19 -> 20 -> 19."""
    (keys, vals), want = many_rows()
    with Context(hasher=0, **dict(SMALL, index_log2=19)) as ctx:
        ctx.index_load(keys, vals)
        assert same_dump(ctx.index_dump(), want)
        for log2 in (20, 19):
            ctx.index_resize(log2)
            assert ctx.index_info() == info_of(log2, 250_000)
            got = ctx.index_dump()
            assert got[0].shape == want[0].shape and same_dump(got, want)
        for i in (0, 1, 124_999, 249_999):                        # and the table still answers
            assert ctx.index_get(bytes(want[0][i])) == bytes(want[1][i])


@gpu
def test_durable_containers_compressor_2():
    """6. retain_containers with Lz4Codec containers: closed, undrained containers and the allocator
    live through the resize; every drained file equals the oracle's."""
    from oracle.oracle import Oracle
    cmax = 1 << 20
    base = make_block("random", 1300, 2 << 20)
    blocks = [base, make_block("random", 1301, 2 << 20), make_block("text", 1302, 2 << 20),
              np.concatenate([base[:1 << 20], make_block("random", 1303, 1 << 20)]),
              make_block("binary", 1304, 2 << 20), make_block("random", 1305, 2 << 20)]
    ids = [9100 + i for i in range(len(blocks))]
    with Context(compressor=2, container_max=cmax, max_block_bytes=4 << 20, max_batch_blocks=1, index_log2=14,
                 arena_slots=32, retain_containers=1) as ctx:
        ora = Oracle(compressor=2, max_size=cmax)
        disk = {}
        for b, i in zip(blocks[:3], ids[:3]):
            compare_block(ctx.reduce_block(b, i), ora.reduce(b, i), tag=f"block {i}")
        assert ctx.stats()["closed_containers"] > 0               # closed and not drained yet
        alloc = ctx.allocator()
        entries = ctx.index_info()["entries"]
        ctx.index_resize(15)
        assert ctx.allocator() == alloc == ora.allocator()
        assert ctx.index_info() == info_of(15, entries)
        first = ctx.drain_containers(buf_bytes=1 << 20)
        assert any(closed for _, closed, _, _ in first)
        _apply(disk, first)
        for b, i in zip(blocks[3:], ids[3:]):
            compare_block(ctx.reduce_block(b, i), ora.reduce(b, i), tag=f"block {i}")
            _apply(disk, ctx.drain_containers(buf_bytes=1 << 20))
        assert ctx.drain_containers() == []
        alloc = ora.allocator()
        n_cont = 0
        for t in range(3):
            for cid in range(t << 22, int.from_bytes(alloc[3 * t:3 * t + 3], "big") + 1):
                od, oc = ora.container(cid)
                if od is None:
                    continue
                n_cont += 1
                assert cid in disk and bytes(disk[cid][0]) == bytes(od) and disk[cid][1] == oc, f"container {cid}"
        assert n_cont == len(disk) > 3
        compare_state(ctx, ora, ids, tag="durable", containers=False)


@gpu
def test_with_a_receive_open():
    """7. A block arrives as packets while the table is resized between two of them."""
    from oracle.oracle import Oracle
    kw = dict(SMALL, index_log2=12)
    blk0, blk = make_block("random", 1400, 600_000), np.ascontiguousarray(make_block("text", 1401, 1_000_000))
    with Context(**kw) as ctx:
        ora = Oracle(max_size=kw["container_max"])
        compare_block(ctx.reduce_block(blk0, 1), ora.reduce(blk0, 1), tag="before")
        rx = ctx.rx_begin(2)
        packets = [np.ascontiguousarray(blk[o:o + 65536]) for o in range(0, len(blk), 65536)]
        for p in packets[:len(packets) // 2]:
            ctx.append_packet(rx, p.ctypes.data, len(p))
        entries = ctx.index_info()["entries"]
        ctx.index_resize(13)
        assert ctx.index_info() == info_of(13, entries)
        for p in packets[len(packets) // 2:]:
            ctx.append_packet(rx, p.ctypes.data, len(p))
        ctx.submit_slot(rx)
        ctx.wait_batch()
        compare_block(ctx.batch_result(0), ora.reduce(blk, 2), tag="received across the resize")
        compare_state(ctx, ora, [1, 2], tag="receive")


@gpu
def test_reset_afterwards():
    """8. hdrf_reset after a grow: an empty index in the grown table, and a fresh DataNode's first block."""
    from oracle.oracle import Oracle
    with Context(hasher=0, **SMALL) as ctx:
        build(ctx, 0)
        ctx.index_resize(12)
        ctx.reset()
        assert ctx.index_count() == 0
        assert ctx.index_info() == info_of(12, 0)
        ora = Oracle(max_size=SMALL["container_max"])
        blk = make_block("random", 1500, 500_000)
        compare_block(ctx.reduce_block(blk, 5), ora.reduce(blk, 5), tag="after reset")
        compare_state(ctx, ora, [5], tag="after reset")


@gpu
def test_node_global_contexts_are_unsupported():
    """9."""
    with Context(n_ranks=2, rank=0, max_block_bytes=1 << 20, max_batch_blocks=2, index_log2=16, arena_slots=16,
                 container_max=1 << 21) as ctx:
        refused(-6, ctx.index_resize, 17)


@gpu
def test_probe_stats_after_a_resize():
    """10. The last batch's slots are the old table's: zeros until a batch has completed in the new one."""
    from oracle.oracle import Oracle
    blk1, blk2 = make_block("random", 1600, 300_000), make_block("text", 1601, 200_000)
    ora = Oracle(max_size=SMALL["container_max"])
    n1, n2 = len(ora.reduce(blk1, 1)["offsets"]), len(ora.reduce(blk2, 2)["offsets"])
    assert n1 != n2
    with Context(hasher=0, **dict(SMALL, index_log2=12)) as ctx:
        ctx.reduce_block(blk1, 1)
        assert ctx.probe_stats()[2] == n1
        ctx.index_resize(13)
        assert ctx.probe_stats() == (0, 0, 0)
        ctx.index_resize(13)                                      # a no-op does not bring the stale slots back
        assert ctx.probe_stats() == (0, 0, 0)
        ctx.reduce_block(blk2, 2)
        s, m, c = ctx.probe_stats()
        assert c == n2 and 0 <= m <= s < (1 << 13) * n2
