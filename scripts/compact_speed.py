"""Times of the passes of hdrf_compact (collect, cover, gather, LZ4, commit) on a
hand-built store: 16 loaded containers of 32 MiB carved into chunks of 2..14 KiB, every other chunk
dropped (only the kept ones are in the index), all 16 compacted by one call.  The library times each
pass with HIP events around its launches (HDRF_COMPACT_TIMES=1 prints them to stderr); the store is
rebuilt before every call, the first one is the warm-up, and the median of the other five is
reported.  The gather's rate (bytes read + bytes written) is printed beside the 6.3 TB/s a streaming
copy reaches on the MI355X (§13c); scripts/read_speed.py, run beside this script, gives the
whole-block read rate of §13b to hold it against.

usage: compact_speed.py [compressor [containers [container_mib]]]      (default 1, 16, 32)"""
import datetime
import os
import re
import statistics
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from hdrf_amd.lib import Context  # noqa: E402

HBM_COPY = 6.3e12


def main():
    comp = int(sys.argv[1]) if len(sys.argv) > 1 else 1
    ncont = int(sys.argv[2]) if len(sys.argv) > 2 else 16
    cmax = (int(sys.argv[3]) if len(sys.argv) > 3 else 32) << 20
    rng = np.random.default_rng(20261021)
    # half of each 4 KiB page is text-like, so the LZ4 pass has matches to find
    data = rng.integers(0, 256, size=cmax, dtype=np.uint8)
    pages = data.reshape(-1, 4096)
    pages[:, 2048:] = pages[:, 2048:] % 23 + 97
    keys, vals, kept_bytes = [], [], 0
    for c in range(ncont):
        lens = rng.integers(2048, 14336, size=cmax // 2048, dtype=np.int64)
        stop = np.cumsum(lens)
        stop = stop[stop <= cmax]
        start = np.concatenate([[0], stop[:-1]])
        start, stop = start[0::2].astype(np.uint32), stop[0::2].astype(np.uint32)     # every other chunk is kept
        v = np.zeros((len(start), 11), np.uint8)
        v[:, 0] = 1
        v[:, 3] = 10 + c
        for j, sh in enumerate((16, 8, 0)):
            v[:, 4 + j] = (start >> sh) & 0xFF
            v[:, 7 + j] = (stop >> sh) & 0xFF
        v[:, 10] = ((start >> 20) & 0xF0) | ((stop >> 24) & 0x0F)
        vals.append(v)
        keys.append(rng.integers(0, 256, size=(len(start), 20), dtype=np.uint8))
        kept_bytes += int((stop - start).sum())
    keys, vals = np.concatenate(keys), np.concatenate(vals)
    ids = [10 + c for c in range(ncont)]
    os.environ["HDRF_COMPACT_TIMES"] = "1"
    log = tempfile.TemporaryFile()
    saved = os.dup(2)
    ctx = Context(hasher=0, compressor=comp, max_block_bytes=1 << 20, max_batch_blocks=2, index_log2=20, arena_slots=8,
                  container_max=cmax)
    for _ in range(6):
        ctx.reset()
        ctx.index_load(keys, vals)
        for cid in ids:
            ctx.container_load(cid, data, lz4=False)
        sys.stderr.flush()
        os.dup2(log.fileno(), 2)                       # the library prints its event times to stderr
        try:
            rows, _ = ctx.compact(ids, want_files=False)
        finally:
            os.dup2(saved, 2)
        assert [r["status"] for r in rows] == [0] * ncont, rows
        assert sum(r["new_bytes"] for r in rows) == kept_bytes
    ctx.close()
    log.seek(0)
    found = re.findall(r"collect ([\d.]+) ms, cover ([\d.]+) ms, gather ([\d.]+) ms, lz4 ([\d.]+) ms, commit ([\d.]+) ms "
                       r"\(containers (\d+), rows (\d+)", log.read().decode())
    runs = [tuple(float(x) for x in r[:5]) for r in found][1:]     # (the first call is the warm-up)
    assert len(runs) == 5, found
    med = [statistics.median(r[i] for r in runs) for i in range(5)]
    print(f"{datetime.date.today()}  compressor {comp}, {ncont} loaded containers of {cmax >> 20} MiB, {len(keys)} live entries "
          f"({found[-1][6]} rows), every other chunk dropped: {kept_bytes} of {ncont * cmax} bytes kept, table 2^20 slots")
    print("median of 5 (after a warm-up): collect %.3f ms (two runs over the table), cover %.3f ms, gather %.3f ms, "
          "lz4 %.3f ms, commit %.3f ms" % tuple(med))
    rate = 2 * kept_bytes / (med[2] * 1e-3)
    print(f"gather: {kept_bytes / (med[2] * 1e-3) / 1e9:.1f} GB/s of kept bytes = {rate / 1e12:.2f} TB/s read + written, "
          f"{rate / HBM_COPY:.2f} of the 6.3 TB/s a streaming copy reaches")
    print("all runs (collect, cover, gather, lz4, commit ms):", runs)


if __name__ == "__main__":
    main()
