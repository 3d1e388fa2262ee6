"""Scrub rate: hdrf_scrub over a context filled with config-2 corpus blocks, beside the write path's
SHA stage over the same blocks in the same run.  Both run the same compression over the same chunks:
the SHA stage contiguously and including duplicates, the scrub over the unique chunks in index-table
order (container bytes through per-lane 132-B windows).  Under rocprofv3 --kernel-trace --stats the
split between vf_collect and vf_hash shows where the scrub's time goes.

usage: scrub_speed.py [blocks [hasher]]      (128 MiB blocks, 32 per batch; default 64 blocks, SHA-1)"""
import datetime
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hdrf_amd.corpus import corpus_roots  # noqa: E402
from hdrf_amd.lib import Context  # noqa: E402


def main():
    nb = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    hasher = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    S, seg, B, seed = 128 << 20, 1 << 20, 32, 20251015
    spb = S // seg
    B = min(B, nb)
    assert nb % B == 0
    # every container stays resident (ring arena of 512 x 32 MiB: 16 GiB, half the corpus is duplicates)
    ctx = Context(hasher=hasher, max_block_bytes=S, max_batch_blocks=B, index_log2=25, arena_slots=512, timing=1,
                  keep_recipes=0)
    total = nb * S + 4096
    dev = ctx.dev_alloc(total)
    ctx.corpus_fill(dev, corpus_roots(seed, 500000, nb, spb), nb, spb, seg, seed)
    ctx.stage_times(reset=True)
    for b0 in range(0, nb, B):
        ctx.reduce_batch([dev + (b0 + i) * S for i in range(B)], [S] * B, [total - (b0 + i) * S for i in range(B)],
                         [b0 + i for i in range(B)])
    sha_ms = ctx.stage_times()[2]
    stats = ctx.stats()
    print(f"{datetime.date.today()}  {nb} x 128 MiB config-2 blocks, hasher {hasher}: {stats['chunks']} chunks, "
          f"{stats['new_bytes'] / 2**30:.2f} GiB stored ({stats['new_bytes']} B) of "
          f"{stats['logical_bytes'] / 2**30:.2f} GiB, {ctx.index_count()} index entries", flush=True)
    for r in range(3):
        t = time.perf_counter()
        st, bad = ctx.scrub()
        dt = time.perf_counter() - t
        # (the scrub hashes one chunk per index entry; on this corpus stats.new_bytes, the sum of
        # storeSize, is a few tens of KB above the bytes the entries name, so it is only a bound here)
        assert not bad and st["skipped"] == 0 and st["checked"] == st["entries"] and st["bytes"] <= stats["new_bytes"], st
        print(f"scrub {r}: {st['checked']} chunks, {st['bytes'] / 2**30:.2f} GiB in {dt * 1e3:.1f} ms = "
              f"{st['bytes'] / dt / 1e9:.1f} GB/s    write-path SHA stage: {stats['logical_bytes'] / 2**30:.2f} GiB in "
              f"{sha_ms:.1f} ms = {stats['logical_bytes'] / sha_ms / 1e6:.1f} GB/s", flush=True)
    ctx.dev_free(dev)
    ctx.close()


if __name__ == "__main__":
    main()
