"""Read rate: the batched, ranged read (hdrf_read_batch) beside the whole-block path (hdrf_reconstruct,
one block per call) over the same store in the same run.  config-2 corpus blocks of 128 MiB reduced
with keep_recipes = 1, then
  (a) every block whole through the hdrf_reconstruct loop (what bench.py's read_bench times)
  (b) every block whole through hdrf_read_batch, 8 and 32 requests per call
  (c) 4,096 seeded 64 KiB ranges: hdrf_read_batch at 256 per call, and whole-block hdrf_reconstruct
      (the reference's shape: rebuild the block, then seek)
  (d) one 128 MiB block of bytes >= 0x80 (forced cuts: 1,000,001-B chunks), both ways
  (e) (b) at 32 per call for T = 4, 8 and 16 KiB (HDRF_READ_TILE)
  (f) hdrf_seek_build of every block, 256 ids per call (the blocks' ids in turn), in ms per id
  (g) (b) and (c) again with the seek tables built: same run, same requests; the table-less legs above run
      code the tables do not touch.  With each (c) leg, the chunk rows of its last call (hdrf_seek_info's
      last_rows) and the 16 B per row they take in the read scratch: the row array by the layout's
      arithmetic, not the scratch's capacity read back (the scratch never shrinks within a run)
Each leg runs three times; all three times are printed (DESIGN.md reports the last two).  Both paths
are called through ctypes with their arguments built beforehand, so the times are the C-ABI's.

usage: read_speed.py [blocks [ranges]]      (default 64 blocks, 4096 ranges)"""
import ctypes
import datetime
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hdrf_amd.corpus import corpus_roots  # noqa: E402
from hdrf_amd.lib import READ_MAX_REQS, Context, ReadReq  # noqa: E402

_u8p = ctypes.POINTER(ctypes.c_uint8)


def timed(label, nbytes, fn, runs=3):
    out = []
    for _ in range(runs):
        t = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t)
    print(f"{label:<58} " + "  ".join(f"{dt * 1e3:9.2f} ms {nbytes / dt / 1e9:8.1f} GB/s" for dt in out), flush=True)
    return out


def main():
    nb = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    nr = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
    S, seg, seed = 128 << 20, 1 << 20, 20251015
    spb = S // seg
    B = min(32, nb)
    assert nb % B == 0
    ctx = Context(hasher=0, max_block_bytes=S, max_batch_blocks=B, index_log2=25, arena_slots=512, keep_recipes=1)
    L, h = ctx.L, ctx._h
    total = nb * S + 4096
    dev = ctx.dev_alloc(total)
    ctx.corpus_fill(dev, corpus_roots(seed, 500000, nb, spb), nb, spb, seg, seed)
    for b0 in range(0, nb, B):
        ctx.reduce_batch([dev + (b0 + i) * S for i in range(B)], [S] * B, [total - (b0 + i) * S for i in range(B)],
                         [b0 + i for i in range(B)])
    st = ctx.stats()
    print(f"{datetime.date.today()}  {nb} x 128 MiB config-2 blocks, SHA-1: {st['chunks']} chunks "
          f"(mean {st['logical_bytes'] / st['chunks']:.0f} B), {st['new_bytes'] / 2**30:.2f} GiB stored", flush=True)
    first = ctx.d2h(dev, S)
    ctx.dev_free(dev)                                      # the reads need only the store
    recipes = [np.frombuffer(ctx.recipe(b), np.uint8).copy() for b in range(nb)]
    out = ctx.dev_alloc(B * S + 4096)

    def reconstruct(b, dst=None):
        r = recipes[b]
        rc = L.hdrf_reconstruct(h, r.ctypes.data_as(_u8p), r.size, out if dst is None else dst, S)
        assert rc == S, rc

    def batches(reqs, per):
        """(ReadReq array, n) per call, built once."""
        calls = []
        for c0 in range(0, len(reqs), per):
            part = reqs[c0:c0 + per]
            arr = (ReadReq * len(part))()
            for q, (bid, off, length, dst) in zip(arr, part):
                q.block_id, q.offset, q.length, q.dev_out = bid, off, length, dst
            calls.append((arr, len(part)))
        return calls

    def run(calls, want):
        for arr, n in calls:
            rc = L.hdrf_read_batch(h, n, arr)
            assert rc == 0 and all(q.result == want for q in arr), rc

    whole = {per: batches([(b, 0, S, out + (b % per) * S) for b in range(nb)], per) for per in (8, 32) if per <= B}
    run(whole[B if B in whole else 8][:1], S)              # warm-up, and the bytes
    assert np.array_equal(ctx.d2h(out, S), first), "block 0 through hdrf_read_batch differs"
    reconstruct(0)
    assert np.array_equal(ctx.d2h(out, S), first), "block 0 through hdrf_reconstruct differs"

    timed("(a) whole blocks, hdrf_reconstruct, one per call", nb * S, lambda: [reconstruct(b) for b in range(nb)])
    for per, calls in whole.items():
        timed(f"(b) whole blocks, hdrf_read_batch, {per} per call", nb * S, lambda: run(calls, S))
    timed("(a) again", nb * S, lambda: [reconstruct(b) for b in range(nb)])

    rng = np.random.default_rng(seed)
    R = 64 << 10
    picks = [(int(rng.integers(nb)), int(rng.integers(0, S - R + 1))) for _ in range(nr)]
    ranged = batches([(b, off, R, out + (i % READ_MAX_REQS) * R) for i, (b, off) in enumerate(picks)], READ_MAX_REQS)
    timed(f"(c) {nr} x 64 KiB ranges, hdrf_read_batch, 256 per call", nr * R, lambda: run(ranged, R))
    timed(f"(c) {nr} x 64 KiB ranges, whole-block hdrf_reconstruct", nr * R, lambda: [reconstruct(b) for b, _ in picks])

    forced = np.random.default_rng(7).integers(0, 256, S, dtype=np.uint8) | 0x80
    fid = nb + 1000
    ctx.reduce_block(forced, fid)
    recipes.append(np.frombuffer(ctx.recipe(fid), np.uint8).copy())
    nch = (recipes[-1].size - 4) // ctx.H
    one = batches([(fid, 0, S, out)], 1)
    run(one, S)
    assert np.array_equal(ctx.d2h(out, S), forced), "the forced-cut block through hdrf_read_batch differs"
    timed(f"(d) one forced-cut block ({nch} chunks), hdrf_read_batch", S, lambda: run(one, S))
    timed(f"(d) one forced-cut block ({nch} chunks), hdrf_reconstruct", S, lambda: reconstruct(nb))

    def rows_note(label):
        info = ctx.seek_info()
        print(f"    {label}: last call {info['last_seek_reqs']} requests from tables, {info['last_rows']} chunk rows = "
              f"{info['last_rows'] * 16 / 2**20:.2f} MiB of row scratch", flush=True)

    run(ranged[-1:], R)
    rows_note("(c) without tables")
    ids = np.array([i % nb for i in range(READ_MAX_REQS)], np.uint64)
    res = (ctypes.c_int32 * READ_MAX_REQS)()

    def build_tables():
        rc = L.hdrf_seek_build(h, ids.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), READ_MAX_REQS, res)
        assert rc == 0 and not any(res), rc

    dts = timed(f"(f) hdrf_seek_build, {READ_MAX_REQS} ids per call", READ_MAX_REQS * S, build_tables)
    print("    " + "  ".join(f"{dt * 1e3 / READ_MAX_REQS:.3f} ms per 128 MiB block" for dt in dts), flush=True)
    ctx.seek_drop(None)
    assert ctx.seek_build(list(range(nb))) == [0] * nb
    info = ctx.seek_info()
    print(f"    tables: {info['blocks']} blocks, {info['chunks']} chunks, store {info['bytes'] / 2**20:.0f} MiB", flush=True)
    run(whole[B if B in whole else 8][:1], S)
    assert np.array_equal(ctx.d2h(out, S), first), "block 0 through the seek path differs"
    for per, calls in whole.items():
        timed(f"(g) as (b) with tables, {per} per call", nb * S, lambda: run(calls, S))
    timed(f"(g) as (c) with tables, {nr} x 64 KiB ranges, 256 per call", nr * R, lambda: run(ranged, R))
    rows_note("(c) with tables")
    b0, off0 = picks[(len(ranged) - 1) * READ_MAX_REQS]
    reconstruct(b0, out + READ_MAX_REQS * R)
    assert np.array_equal(ctx.d2h(out, R), ctx.d2h(out + READ_MAX_REQS * R + off0, R)), "a ranged read through the seek path differs"
    ctx.seek_drop(None)
    timed("(c) again without tables", nr * R, lambda: run(ranged, R))

    if B in whole:
        for kib in (4, 8, 16):
            os.environ["HDRF_READ_TILE"] = str(kib << 10)
            timed(f"(e) as (b) {B} per call, T = {kib} KiB", nb * S, lambda: run(whole[B], S))
            timed(f"(e) as (d) hdrf_read_batch, T = {kib} KiB", S, lambda: run(one, S))
        os.environ.pop("HDRF_READ_TILE")
    ctx.dev_free(out)
    ctx.close()


if __name__ == "__main__":
    main()
