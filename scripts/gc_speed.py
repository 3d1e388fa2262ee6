"""Times of the three passes of hdrf_gc (mark, sweep, rebuild) on a hand-built store:
an index of `entries` synthetic rows (random digests, 256 containers) in a table of 2^index_log2 slots,
`entries / 1024` recipes of 1024 digests each that cover every row once, every other recipe deleted.
The library times each pass with HIP events around its launches (HDRF_GC_TIMES=1 prints them to
stderr); the store is rebuilt before every collection, the first one is the warm-up, and the median of
the other five is reported, with the sweep's table bytes per second beside the HBM rates of the MI355X
(8.0 TB/s specified, 6.3 TB/s reached by a streaming copy).

usage: gc_speed.py [index_log2 [entries [hasher]]]      (default 24, 8 Mi, SHA-1)"""
import datetime
import os
import re
import statistics
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from hdrf_amd.lib import Context  # noqa: E402

PER = 1024          # digests per recipe
HBM_SPEC, HBM_COPY = 8.0e12, 6.3e12


def main():
    log2 = int(sys.argv[1]) if len(sys.argv) > 1 else 24
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 8 << 20
    hasher = int(sys.argv[3]) if len(sys.argv) > 3 else 0
    H = 20 if hasher == 0 else 28
    assert n % PER == 0 and n < (1 << log2)
    rng = np.random.default_rng(20261021)
    keys = rng.integers(0, 256, size=(n, H), dtype=np.uint8)
    cid = rng.integers(0, 256, size=n, dtype=np.uint32)
    start = rng.integers(0, 1 << 24, size=n, dtype=np.uint32)
    stop = start + rng.integers(64, 4096, size=n, dtype=np.uint32)
    vals = np.zeros((n, 11), np.uint8)
    vals[:, 0] = 1
    vals[:, 3] = cid
    for j, sh in enumerate((16, 8, 0)):
        vals[:, 4 + j] = (start >> sh) & 0xFF
        vals[:, 7 + j] = (stop >> sh) & 0xFF
    vals[:, 10] = ((start >> 20) & 0xF0) | ((stop >> 24) & 0x0F)
    nrec = n // PER
    recipes = [(PER * 1000).to_bytes(4, "big") + keys[j * PER:(j + 1) * PER].tobytes() for j in range(nrec)]
    os.environ["HDRF_GC_TIMES"] = "1"
    log = tempfile.TemporaryFile()
    saved = os.dup(2)
    ctx = Context(hasher=hasher, max_block_bytes=1 << 20, max_batch_blocks=2, index_log2=log2, arena_slots=8,
                  container_max=1 << 21)
    stats = None
    for _ in range(6):
        ctx.reset()
        ctx.index_load(keys, vals)
        for j, r in enumerate(recipes):
            ctx.recipe_load(j, r)
        for j in range(0, nrec, 2):
            ctx.block_delete(j)
        sys.stderr.flush()
        os.dup2(log.fileno(), 2)                       # the library prints its event times to stderr
        try:
            st = ctx.L.hdrf_gc(ctx._h, 0, None, None, 0)
        finally:
            os.dup2(saved, 2)
        assert st == 256, st
        stats, _ = ctx.gc(dry=True)
        assert stats["entries"] == stats["kept"] == n // 2 and stats["dropped"] == 0, stats
    ctx.close()
    log.seek(0)
    rows = re.findall(r"mark ([\d.]+) ms, sweep ([\d.]+) ms, rebuild ([\d.]+) ms", log.read().decode())
    runs = [tuple(float(x) for x in r) for r in rows][1:]          # (the first collection is the warm-up)
    assert len(runs) == 5, rows
    mark, sweep, rebuild = (statistics.median(r[i] for r in runs) for i in range(3))
    table = 64 << log2
    print(f"{datetime.date.today()}  index_log2 {log2}, {n} live entries, hasher {hasher}, {nrec} recipes x {PER} digests, "
          f"every other recipe deleted: {n // 2} kept, {n // 2} dropped")
    print(f"median of 5 (after a warm-up): mark {mark:.3f} ms ({n // 2} digests), sweep {sweep:.3f} ms "
          f"({table / 2**20:.0f} MiB of table), rebuild {rebuild:.3f} ms ({n // 2} rows)")
    rate = table / (sweep * 1e-3)
    print(f"sweep: {rate / 1e12:.2f} TB/s of table = {rate / HBM_SPEC:.2f} of the 8.0 TB/s HBM specification, "
          f"{rate / HBM_COPY:.2f} of the 6.3 TB/s a streaming copy reaches")
    print("all runs (mark, sweep, rebuild ms):", runs)


if __name__ == "__main__":
    main()
