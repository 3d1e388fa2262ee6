"""Times of hdrf_index_resize against the path the table's growth took before it:
dump the index to the host, close the context, open one with index_log2 + 1, load the index again.

The store is an index of `entries` synthetic rows (random digests) in a table of 2^index_log2 slots:
by default 10,000,000 rows in 2^24 slots, 60 % load, the line at which DESIGN.md §7b says to grow.

Direct: the table goes 24 -> 25 -> 24 -> ... ; the library times its passes with HIP events around
their launches (HDRF_RESIZE_TIMES=1 prints them to stderr), the first grow and the first shrink are the
warm-up, and the median of the other `runs` of each direction is reported, with the rehash's rate
against the bytes it must move (the old table read + 64 B written per live entry) beside the HBM rates
of the MI355X (8.0 TB/s specified, 6.3 TB/s reached by a streaming copy).  The whole call — allocation
of the new table and release of the old one included — is timed with the host clock around it (the
call ends in a device synchronise).
Baseline: hdrf_index_dump, hdrf_close, hdrf_open with index_log2 + 1, hdrf_index_load, timed with the
host clock, one warm-up and `runs` runs.  The baseline is charged nothing for what it loses besides:
recipes, the allocator, the containers and the receive buffers would have to be reloaded too.

usage: index_resize_speed.py [index_log2 [entries [runs [baseline_runs]]]]      (default 24, 10,000,000, 5, 5)"""
import ctypes
import datetime
import os
import re
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from hdrf_amd.lib import Context, _p  # noqa: E402

HBM_SPEC, HBM_COPY = 8.0e12, 6.3e12
CFG = dict(hasher=0, max_block_bytes=1 << 20, max_batch_blocks=2, arena_slots=8, container_max=1 << 21)


def rows(n):
    rng = np.random.default_rng(20261021)
    keys = rng.integers(0, 256, size=(n, 20), dtype=np.uint8)
    vals = rng.integers(0, 256, size=(n, 11), dtype=np.uint8)
    return keys, vals


def spread(xs):
    return f"{min(xs):.3f} .. {max(xs):.3f}"


def direct(log2, keys, vals, runs):
    n = len(keys)
    os.environ["HDRF_RESIZE_TIMES"] = "1"
    log = tempfile.TemporaryFile()
    saved = os.dup(2)
    wall = {log2 + 1: [], log2: []}
    with Context(index_log2=log2, **CFG) as ctx:
        ctx.index_load(keys, vals)
        assert ctx.index_info()["entries"] == n
        for _ in range(runs + 1):
            for to in (log2 + 1, log2):
                sys.stderr.flush()
                os.dup2(log.fileno(), 2)                   # the library prints its event times to stderr
                try:
                    t0 = time.perf_counter()
                    rc = ctx.L.hdrf_index_resize(ctx._h, to)
                    wall[to].append((time.perf_counter() - t0) * 1e3)
                finally:
                    os.dup2(saved, 2)
                assert rc == 0, rc
        info = ctx.index_info()
        assert info["entries"] == n and info["index_log2"] == log2
        for i in (0, n // 2, n - 1):                       # and the table still answers
            assert ctx.index_get(keys[i].tobytes()) is not None
    os.environ.pop("HDRF_RESIZE_TIMES")
    log.seek(0)
    pat = (r"count ([\d.]+) ms, clear ([\d.]+) ms, rehash ([\d.]+) ms, recount ([\d.]+) ms "
           r"\(log2 (\d+) -> (\d+), entries (\d+), rehash bytes (\d+)\)")
    got = [(int(m[4]), int(m[5]), int(m[7]), [float(x) for x in m[:4]]) for m in re.findall(pat, log.read().decode())]
    assert len(got) == 2 * (runs + 1), got
    for a, b, name in ((log2, log2 + 1, "grow"), (log2 + 1, log2, "shrink")):
        mine = [g for g in got if (g[0], g[1]) == (a, b)][1:]              # (the first is the warm-up)
        assert len(mine) == runs
        nbytes = mine[0][2]
        assert nbytes == (64 << a) + 64 * n
        cols = list(zip(*(g[3] for g in mine)))
        med = [statistics.median(c) for c in cols]
        w = wall[b][1:]
        print(f"{name} {a} -> {b}, median of {runs} (after a warm-up): count {med[0]:.3f} ms ({(64 << a) >> 20} MiB), "
              f"clear {med[1]:.3f} ms ({(64 << b) >> 20} MiB), rehash {med[2]:.3f} ms, recount {med[3]:.3f} ms "
              f"({(64 << b) >> 20} MiB); passes {sum(med):.3f} ms")
        print(f"  spread (min .. max ms): count {spread(cols[0])}, clear {spread(cols[1])}, rehash {spread(cols[2])}, "
              f"recount {spread(cols[3])}")
        rate = nbytes / (med[2] * 1e-3)
        print(f"  rehash: {nbytes} B to move (old table read {64 << a} + {n} live x 64 written) = {rate / 1e12:.2f} TB/s = "
              f"{rate / HBM_SPEC:.2f} of the 8.0 TB/s HBM specification, {rate / HBM_COPY:.2f} of the 6.3 TB/s a "
              f"streaming copy reaches; at 6.3 TB/s those bytes take {nbytes / HBM_COPY * 1e3:.3f} ms, so "
              f"{med[2] - nbytes / HBM_COPY * 1e3:.3f} ms is the claims' share ({n} compare-and-swaps, "
              f"{n / (med[2] * 1e-3) / 1e9:.2f} G claims/s)")
        print(f"  whole call (host clock, new table's allocation and old table's release included): median "
              f"{statistics.median(w):.3f} ms, {spread(w)}")
        print(f"  all runs (count, clear, rehash, recount ms): {[g[3] for g in mine]}")
        if name == "grow":
            grow_call = statistics.median(w)
            grow_passes = sum(med)
    return grow_call, grow_passes


def baseline(log2, keys, vals, runs):
    n = len(keys)
    parts = []
    for _ in range(runs + 1):
        ctx = Context(index_log2=log2, **CFG)
        ctx.index_load(keys, vals)
        ctx.synchronize()
        k = np.zeros(n * 20, np.uint8)
        v = np.zeros(n * 11, np.uint8)
        t0 = time.perf_counter()
        got = ctx.L.hdrf_index_dump(ctx._h, _p(k), _p(v), n)
        t1 = time.perf_counter()
        ctx.close()
        t2 = time.perf_counter()
        new = Context(index_log2=log2 + 1, **CFG)
        t3 = time.perf_counter()
        new.index_load(k, v)
        new.synchronize()
        t4 = time.perf_counter()
        assert got == n and new.index_info() == dict(index_log2=log2 + 1, slots=2 << log2, entries=n,
                                                     table_bytes=128 << log2)
        new.close()
        parts.append([(b - a) * 1e3 for a, b in ((t0, t1), (t1, t2), (t2, t3), (t3, t4), (t0, t4))])
    parts = parts[1:]
    cols = list(zip(*parts))
    med = [statistics.median(c) for c in cols]
    print(f"baseline {log2} -> {log2 + 1} (dump, close, open, load; host clock), median of {runs} (after a warm-up): "
          f"dump {med[0]:.1f} ms, close {med[1]:.1f} ms, open {med[2]:.1f} ms, load {med[3]:.1f} ms; total {med[4]:.1f} ms "
          f"({spread(cols[4])})")
    print(f"  all runs (dump, close, open, load, total ms): {[[round(x, 1) for x in p] for p in parts]}")
    return med[4]


def main():
    log2 = int(sys.argv[1]) if len(sys.argv) > 1 else 24
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 10_000_000
    runs = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    bruns = int(sys.argv[4]) if len(sys.argv) > 4 else 5
    assert 10 <= log2 <= 30 and n * 4 <= 3 << log2, "the rows must fit the smaller table under the 75 % rule"
    keys, vals = rows(n)
    print(f"{datetime.date.today()}  index_log2 {log2}, {n} live entries ({n / (1 << log2):.3f} load), SHA-1")
    call, passes = direct(log2, keys, vals, runs)
    base = baseline(log2, keys, vals, bruns)
    print(f"grow {log2} -> {log2 + 1}: baseline {base:.1f} ms / direct call {call:.3f} ms = {base / call:.0f}x "
          f"(/ its four passes alone, {passes:.3f} ms: {base / passes:.0f}x)")


if __name__ == "__main__":
    main()
