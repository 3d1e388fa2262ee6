"""Fingerprint scrub (hdrf_scrub) and verified reads (hdrf_reconstruct*_verified): stored chunks
re-hashed on the GPU and compared with the digest that names them.  Expected results come from
hashlib and plain Python over the test's own bytes, never from the code under test."""
import ctypes
import hashlib
import os
import subprocess

import numpy as np
import pytest

from helpers import make_block, prng_bytes
from hdrf_amd.lib import BadChunk, Context, HdrfError, ScrubStats, load

gpu = pytest.mark.gpu

HASH = {0: hashlib.sha1, 1: hashlib.sha224}
CID = 5                                   # the hand-built store's container
CFG = dict(max_block_bytes=4 << 20, max_batch_blocks=2, index_log2=16, arena_slots=16, container_max=4 << 20)


# ---- CPU: the ABI -----------------------------------------------------------------------------
def test_struct_sizes_match_the_c_static_asserts():
    """sizeof(hdrf_bad_chunk) == 44 and sizeof(hdrf_scrub_stats) == 40 (api_verify.hip)."""
    assert ctypes.sizeof(BadChunk) == 44
    assert ctypes.sizeof(ScrubStats) == 40
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hdrf_amd", "csrc",
                            "api_verify.hip")).read()
    assert "static_assert(sizeof(hdrf_bad_chunk) == 44" in src
    assert "static_assert(sizeof(hdrf_scrub_stats) == 40" in src


def test_null_context_is_invalid():
    L = load()
    st = ScrubStats()
    assert L.hdrf_scrub(None, -1, None, 0, ctypes.byref(st)) == -1
    bad = ctypes.c_int64(0)
    rec = (ctypes.c_uint8 * 24)()
    assert L.hdrf_reconstruct_verified(None, rec, 24, None, 0, ctypes.byref(bad)) == -1
    assert L.hdrf_reconstruct_block_verified(None, 1, None, 0, ctypes.byref(bad)) == -1


def test_entry_codec_under_asan_and_ubsan(tmp_path):
    """tests/cpp/entry_codec_test.cpp: an entry's digest packing against its inverse for both hashers, and
    the 11-byte value against chunkMeta.getMeta byte by byte, as a plain program built with
    -fsanitize=address,undefined."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "entry_codec_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(root, "tests", "cpp", "entry_codec_test.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "PASS" in r.stdout


# ---- helpers ----------------------------------------------------------------------------------
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


def test_value_encoder_round_trips():
    for cid, start, stop in [(0, 0, 0), (CID, 1, 2), (0x812345, 0x1ABCDEF, 0x1FFFFFF), (3 << 22, 0xFFFFFF, 0x1000000)]:
        assert dec_value(enc_value(7, cid, start, stop)) == (cid, start, stop)


FIXED = [0, 1, 3, 55, 56, 57, 63, 64, 65, 119, 120, 127, 128, 129, 191, 192, 700, 701, 4096, 65535, 65536, 65537,
         1_000_000]


def chunk_lengths():
    """The fixed lengths (every FIPS padding boundary, the pair alignment, both sides of the long-chunk
    threshold, a full forced-cut chain), then 300 from a fixed sequence in [700, 5000]."""
    out = list(FIXED)
    x = 12345
    for _ in range(300):
        x = (x * 1103515245 + 12345) & 0x7FFFFFFF
        out.append(700 + (x >> 8) % 4301)
    return out


_STORES = {}


def hand_store(hasher):
    """(file bytes, rows): one raw container carved back to back into chunks; rows = (digest,
    container, start, stop) in file order.  The last chunk ends at the file's last byte."""
    if hasher not in _STORES:
        lens = chunk_lengths()
        data = prng_bytes(4242, sum(lens)).tobytes()
        rows, pos = [], 0
        for n in lens:
            rows.append((HASH[hasher](data[pos:pos + n]).digest(), CID, pos, pos + n))
            pos += n
        assert pos == len(data)
        assert len({r[0] for r in rows}) == len(rows)
        assert {r[2] & 3 for r in rows} == {0, 1, 2, 3}          # all four start alignments
        _STORES[hasher] = (data, rows)
    return _STORES[hasher]


def load_rows(ctx, rows):
    keys = np.frombuffer(b"".join(r[0] for r in rows), np.uint8)
    vals = np.frombuffer(b"".join(enc_value(1, r[1], r[2], r[3]) for r in rows), np.uint8)
    ctx.index_load(keys, vals)


def as_set(bad):
    return sorted((b["container"], b["start"], b["digest"], b["stop"], b["why"]) for b in bad)


def expect(rows, why):
    return sorted((r[1], r[2], r[0], r[3], why) for r in rows)


def check_sorted(bad):
    k = [(b["container"], b["start"], b["digest"]) for b in bad]
    assert k == sorted(k)


@pytest.fixture(params=[None, 1], ids=["device-grid", "one-workgroup"])
def grid(request, monkeypatch):
    """The hash kernel's grid.  A wave reserves 64 items at a time, so on the device-sized grid
    (about 2048 waves) no wave of these small stores reserves twice.  With one workgroup (4 waves,
    HDRF_VF_WGS=1) the waves consume the whole store: second and later reservations, hand-out from
    a partly used pool (lane refill), a refill inside one pass, and the 1,000,000-B chunk's lane
    busy while its wave's other lanes go through item after item."""
    if request.param is not None:
        monkeypatch.setenv("HDRF_VF_WGS", str(request.param))
    return request.param


# ---- GPU ------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("hasher", [0, 1])
def test_hand_built_store_is_clean(hasher, grid):
    data, rows = hand_store(hasher)
    with Context(hasher=hasher, **CFG) as ctx:
        load_rows(ctx, rows)
        ctx.container_load(CID, data, lz4=False)
        st, bad = ctx.scrub()
        print("clean scrub:", st)
        assert bad == [] and st["bad"] == 0
        assert st["checked"] == st["entries"] == len(rows)
        assert st["skipped"] == 0
        assert st["bytes"] == sum(r[3] - r[2] for r in rows) == len(data)


@gpu
@pytest.mark.parametrize("hasher", [0, 1])
def test_one_flipped_byte_is_localised(hasher, grid):
    data, rows = hand_store(hasher)
    big = next(r for r in rows if r[3] - r[2] == 1_000_000)
    one = next(r for r in rows if r[3] - r[2] == 1)
    positions = [rows[40][2],                 # a chunk's first byte
                 rows[41][3] - 1,             # a chunk's last byte
                 len(data) - 1,               # the file's last byte
                 rows[60][2] + 64,            # offset 64 inside a chunk
                 (big[2] + big[3]) // 2,      # the middle of the 1,000,000-B chunk
                 one[2]]                      # the 1-B chunk
    with Context(hasher=hasher, **CFG) as ctx:
        load_rows(ctx, rows)
        for pos in positions:
            hit = [r for r in rows if r[2] <= pos < r[3]]
            assert len(hit) == 1
            f = bytearray(data)
            f[pos] ^= 0x40
            ctx.container_load(CID, bytes(f), lz4=False)          # replaces the previous copy
            st, bad = ctx.scrub()
            assert as_set(bad) == expect(hit, 1), f"flip at {pos}"
            assert st["bad"] == 1 and st["checked"] == st["entries"] == len(rows)
            st1, bad1 = ctx.scrub(container=CID)
            assert (st1, bad1) == (st, bad)
        ctx.container_load(CID, data, lz4=False)
        st, bad = ctx.scrub(container=None)
        assert bad == [] and st["bad"] == 0 and st["checked"] == len(rows)
        assert ctx.scrub(container=CID) == (st, bad)


@gpu
@pytest.mark.parametrize("hasher", [0, 1])
def test_ranges_outside_the_container(hasher, grid):
    """Every overrun stays within 32 bytes of the file's end: even an unchecked read would stay inside
    the loaded copy's allocation."""
    data, rows = hand_store(hasher)
    with Context(hasher=hasher, **CFG) as ctx:
        load_rows(ctx, rows)
        cut = len(data) - 10                                      # (a) the file cut short by 10 bytes
        ctx.container_load(CID, data[:cut], lz4=False)
        over = [r for r in rows if r[3] > cut]
        assert over and all(r[3] - cut <= 32 for r in over)
        st, bad = ctx.scrub()
        assert as_set(bad) == expect(over, 2)
        assert st["entries"] == len(rows) and st["checked"] == len(rows) - len(over)
        assert st["bytes"] == sum(r[3] - r[2] for r in rows if r[3] <= cut)
    with Context(hasher=hasher, **CFG) as ctx:                    # (b) one row past the whole file
        extra = (HASH[hasher](b"a row past the end").digest(), CID, len(data) - 100, len(data) + 1)
        load_rows(ctx, rows + [extra])
        ctx.container_load(CID, data, lz4=False)
        st, bad = ctx.scrub()
        assert as_set(bad) == expect([extra], 2)
        assert st["entries"] == len(rows) + 1 and st["checked"] == len(rows)


@gpu
def test_unreadable_containers_are_skipped():
    data, rows = hand_store(0)
    ghost = [(hashlib.sha1(b"ghost %d" % i).digest(), 9, 100 * i, 100 * i + 50) for i in range(3)]
    with Context(hasher=0, **CFG) as ctx:
        load_rows(ctx, rows + ghost)
        ctx.container_load(CID, data, lz4=False)
        st, bad = ctx.scrub()
        assert bad == [] and st["skipped"] == 3
        assert st["entries"] == len(rows) + 3 and st["checked"] == len(rows)
        st, bad = ctx.scrub(container=CID)
        assert bad == [] and st["skipped"] == 0 and st["entries"] == st["checked"] == len(rows)
        with pytest.raises(HdrfError) as e:
            ctx.scrub(container=9)
        assert e.value.code == -5


@gpu
def test_slice_walk_matches_one_slice(monkeypatch):
    """The table walked in 64 slices of 2^10 slots gives what one slice gives (bad rows included)."""
    data, rows = hand_store(0)
    f = bytearray(data)
    flips = [rows[i] for i in (25, 100, 200, 322)]
    for r in flips:
        f[r[2]] ^= 1
    with Context(hasher=0, **CFG) as ctx:
        load_rows(ctx, rows)
        ctx.container_load(CID, bytes(f), lz4=False)
        whole = ctx.scrub()
        monkeypatch.setenv("HDRF_SCRUB_SLICE_LOG2", "10")
        sliced = ctx.scrub()
        assert sliced == whole
        assert as_set(whole[1]) == expect(flips, 1)
        check_sorted(whole[1])
        assert whole[0]["checked"] == len(rows)


def restart_blocks():
    """Blocks built like test_restart_from_persisted_state's: overlapping pieces of three base blocks
    plus fresh random bytes, so that recipes share chunks."""
    rng = np.random.default_rng(3)
    base = [make_block(k, 90 + i, 800_000) for i, k in enumerate(["random", "text", "binary"])]
    blocks = []
    for i in range(8):
        parts = [base[int(rng.integers(3))][int(rng.integers(0, 300_000)):][:250_000] for _ in range(2)]
        blocks.append(np.concatenate(parts + [make_block("random", 700 + i, 300_000)]))
    return blocks


@gpu
@pytest.mark.parametrize("hasher,compressor", [(0, 1), (1, 2)])
def test_real_store_restart_and_verified_reads(hasher, compressor, grid):
    cmax = 1 << 20
    blocks = restart_blocks()
    ids = [3000 + i for i in range(len(blocks))]
    kw = dict(hasher=hasher, compressor=compressor, container_max=cmax, max_block_bytes=16 << 20, max_batch_blocks=8,
              index_log2=20, arena_slots=64)
    H = HASH[hasher]().digest_size
    with Context(**kw) as ctx1:
        for b, i in zip(blocks, ids):
            ctx1.reduce_block(b, i)
        st, bad = ctx1.scrub()
        print("live scrub:", st)
        assert bad == [] and st["bad"] == 0 and st["skipped"] == 0
        assert st["checked"] == ctx1.index_count()
        assert st["bytes"] == ctx1.stats()["new_bytes"]
        keys, vals = ctx1.index_dump()
        alloc = ctx1.allocator()
        recipes = {i: ctx1.recipe(i) for i in ids}
        files = {}
        for t in range(3):
            for cid in range(t << 22, int.from_bytes(alloc[3 * t:3 * t + 3], "big") + 1):
                d, closed = ctx1.container(cid)
                if d is not None:
                    files[cid] = (d, closed)
    assert any(closed for _, closed in files.values())
    with Context(**kw) as ctx2:                                   # the restarted DataNode
        ctx2.index_load(keys, vals)
        for i, r in recipes.items():
            ctx2.recipe_load(i, r)
        for cid, (d, closed) in files.items():
            ctx2.container_load(cid, d, closed and compressor == 2)
        st, bad = ctx2.scrub()
        assert bad == [] and st["checked"] == st["entries"] == len(keys) and st["skipped"] == 0
        for i, b in zip(ids, blocks):
            assert np.array_equal(ctx2.reconstruct_block(i, verify=True), b), f"block {i}"
        dev = ctx2.dev_alloc(len(blocks[0]) + 64)                 # hdrf_reconstruct_verified: output left in HBM
        for off in (0, 1, 3):                                     # ... at any byte alignment
            assert ctx2.reconstruct(recipes[ids[0]], dev + off, len(blocks[0]), verify=True) == len(blocks[0])
            assert np.array_equal(ctx2.d2h(dev + off, len(blocks[0])), blocks[0])
        if compressor != 1:
            ctx2.dev_free(dev)
            return
        # one flipped byte in a closed container file: choose it so that some blocks fail and some pass
        rows = [(bytes(k), *dec_value(v)) for k, v in zip(keys, vals)]
        digs = {i: [r[4 + H * j:4 + H * (j + 1)] for j in range((len(r) - 4) // H)] for i, r in recipes.items()}
        pick = None
        for cid, (d, closed) in sorted(files.items()):
            if not closed:
                continue
            for pos in [len(d) // 2 + s for s in range(0, len(d) // 2, 50_000)]:
                hit = [r for r in rows if r[1] == cid and r[2] <= pos < r[3]]
                users = [i for i in ids if any(h[0] in digs[i] for h in hit)]
                if hit and 0 < len(users) < len(ids):
                    pick = (cid, pos)
                    break
            if pick:
                break
        assert pick, "no byte found that some blocks use and some do not"
        cid, pos = pick
        f = bytearray(files[cid][0])
        f[pos] ^= 0x01
        ctx2.container_load(cid, bytes(f), False)
        fbytes = {c: (bytes(f) if c == cid else d) for c, (d, _) in files.items()}
        want = [r for r in rows if HASH[hasher](fbytes[r[1]][r[2]:r[3]]).digest() != r[0]]
        assert len(want) >= 1
        st, bad = ctx2.scrub()
        assert as_set(bad) == expect(want, 1)
        assert st["bad"] == len(want) and st["checked"] == len(rows)
        baddig = {r[0] for r in want}
        failed = passed = 0
        for i, b in zip(ids, blocks):
            pos_bad = [j for j, dg in enumerate(digs[i]) if dg in baddig]
            if pos_bad:
                with pytest.raises(HdrfError) as e:
                    ctx2.reconstruct_block(i, verify=True)
                assert e.value.code == -8 and e.value.bad_chunk == pos_bad[0]
                assert digs[i][pos_bad[0]].hex() in str(e.value) and f"container {cid}" in str(e.value)
                failed += 1
            else:
                assert np.array_equal(ctx2.reconstruct_block(i, verify=True), b), f"block {i}"
                passed += 1
            got = ctx2.reconstruct_block(i)                       # unverified: bytes, and no error
            assert len(got) == len(b)
            assert np.array_equal(got, b) == (not pos_bad)
            if pos_bad:                                           # the device-output call reports the same
                with pytest.raises(HdrfError) as e:
                    ctx2.reconstruct(recipes[i], dev, len(b), verify=True)
                assert e.value.code == -8 and e.value.bad_chunk == pos_bad[0]
                assert np.array_equal(ctx2.d2h(dev, len(b)), got)     # the bytes are in the output anyway
                assert ctx2.reconstruct(recipes[i], dev, len(b)) == len(b)
        ctx2.dev_free(dev)
        assert failed > 0 and passed > 0


@gpu
def test_scrub_completes_batches_in_flight():
    blocks = [make_block("random", 51, 900_000), make_block("text", 52, 700_001)]
    with Context(hasher=0, **CFG) as ctx:
        ptrs = []
        for b in blocks:
            p = ctx.dev_alloc(len(b) + 64)
            ctx.h2d(p, b)
            ptrs.append(p)
        ctx.submit_batch(ptrs, [len(b) for b in blocks], [len(b) + 64 for b in blocks], [1, 2])
        st, bad = ctx.scrub()                                     # no wait_batch: the scrub completes it
        assert bad == [] and st["bad"] == 0 and st["skipped"] == 0
        assert st["checked"] == ctx.index_count() > 0
        assert st["bytes"] == ctx.stats()["new_bytes"]
        for p in ptrs:
            ctx.dev_free(p)


@gpu
def test_cpp_scheme_scrub_and_verified_read(tmp_path):
    """include/hdrf_scheme.hpp: HipReductionScheme::scrub and ::reconstruct_verified
    (tests/cpp/scrub_scheme_test.cpp)."""
    import hdrf_amd.lib as lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "scrub_scheme_test")
    libdir = os.path.dirname(lib.LIB_PATH)
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(root, "include"),
                    os.path.join(root, "tests", "cpp", "scrub_scheme_test.cpp"), "-o", exe, "-L", libdir, "-lhdrf",
                    "-Wl,-rpath," + libdir], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "PASS" in r.stdout


@gpu
def test_node_global_context_is_unsupported():
    with Context(n_ranks=2, rank=0, max_block_bytes=1 << 20, max_batch_blocks=2, index_log2=16, arena_slots=16,
                 container_max=1 << 21) as ctx:
        with pytest.raises(HdrfError) as e:
            ctx.scrub()
        assert e.value.code == -6
