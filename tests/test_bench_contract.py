"""bench.py bookkeeping that needs no GPU: the per-stream chains match the library's streams and
the committed PMC traffic is attached only to the workload it was measured on."""
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WANT = {"blocks": 512, "block_mib": 128, "batch": 32, "n_gpus": 1, "hasher": 0}


def _bench(monkeypatch, split=None):
    if split is None:
        monkeypatch.delenv("HDRF_SPLIT_B", raising=False)
    else:
        monkeypatch.setenv("HDRF_SPLIT_B", split)
    import bench
    return importlib.reload(bench)


def test_chains_follow_the_split_back_stage(monkeypatch):
    b = _bench(monkeypatch)
    assert list(b.CHAINS) == ["W: chunking", "A: SHA", "B: index", "B2: store", "L: LZ4"]
    assert "place(place_kernel)" in b.CHAINS["B2: store"]
    b = _bench(monkeypatch, "0")
    assert list(b.CHAINS) == ["W: chunking", "A: SHA", "B: index+store", "L: LZ4"]
    stages = [s for c in b.CHAINS.values() for s in c]
    assert len(stages) == len(set(stages))                # every stage timed on exactly one chain
    _bench(monkeypatch)


def test_traffic_is_matched_by_workload(monkeypatch):
    b = _bench(monkeypatch)
    d2, src2 = b.load_pmc(dict(WANT, workload="config2"))
    d4, src4 = b.load_pmc(dict(WANT, workload="config4"))
    assert src2 and src4 and src2 != src4
    assert d4["_config"]["workload"] == "config4"
    assert d2.get("_config", {}).get("workload", "config2") == "config2"
    assert "lz4_seg_kernel<false>" in d4 and "place_kernel<true>" in d2
    assert b.load_pmc(dict(WANT, workload="config5", blocks=128)) == ({}, None)


def test_named_kernels_have_committed_traffic(monkeypatch):
    """Every kernel the config-2 line names (its roofline entries) is in the newest config-2 traffic
    file, so a renamed kernel cannot silently drop the line's `traffic`."""
    b = _bench(monkeypatch)
    d, _ = b.load_pmc(dict(WANT, workload="config2"))
    for name, kern in b.KERNEL_OF.items():
        assert b.pmc_lookup(d, kern).get("hbm_bytes_per_launch"), (name, kern)


def test_plain_run_is_the_default_and_full_is_an_option(monkeypatch):
    b = _bench(monkeypatch)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "3"])
    a = b.parse()
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 3)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out"])
    a = b.parse()
    assert a.full and a.dump_outputs == "out"


class _FakeCtx:
    """The calls dump_outputs makes, answered from fixed arrays (3 blocks in the last batch)."""
    H = 20

    def __init__(self, n):
        import numpy as np
        self.n = n
        self.np = np

    def stats(self):
        return {"blocks": 3, "chunks": 3 * self.n}

    def index_count(self):
        return 17

    def allocator(self):
        return bytes(range(24))

    def last_nblocks(self):
        return 3

    def batch_result(self, i):
        np = self.np
        r = np.random.default_rng(i)
        n = self.n
        return {"offsets": np.sort(r.integers(0, 1 << 27, n)).astype(np.uint32),
                "digests": r.integers(0, 256, (n, self.H)).astype(np.uint8), "is_new": r.integers(0, 2, n).astype(np.uint8),
                "container_id": r.integers(0, 1 << 24, n).astype(np.uint32),
                "container_pos": r.integers(0, 1 << 25, n).astype(np.uint32), "store_size": 0}


def test_dump_outputs_is_exact_repeatable_and_bounded(monkeypatch, tmp_path):
    """--dump-outputs: float32 / float64 arrays that hold the integers exactly, the same files from the
    same results, and a seeded row sample once the per-chunk arrays would pass the budget."""
    import numpy as np
    b = _bench(monkeypatch)
    n_chunks, store = np.array([5, 6, 7], np.int64), np.array([1 << 27, 3, (1 << 27) - 1], np.int64)
    ctx = _FakeCtx(1000)
    b.dump_outputs(str(tmp_path / "a"), ctx, n_chunks, store, 0, 1)
    b.dump_outputs(str(tmp_path / "b"), ctx, n_chunks, store, 0, 1)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    assert {"n_chunks.npy", "store_size.npy", "stats.npy", "allocator.npy", "last_batch_block0_offsets.npy",
            "last_batch_block1_digests.npy", "last_batch_block2_is_new.npy"} <= set(names)
    for f in names:
        x, y = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert x.dtype in (np.float32, np.float64) and np.array_equal(x, y), f
    assert np.array_equal(np.load(tmp_path / "a" / "store_size.npy"), store)
    r = ctx.batch_result(2)
    assert np.array_equal(np.load(tmp_path / "a" / "last_batch_block2_offsets.npy"), r["offsets"])
    assert np.array_equal(np.load(tmp_path / "a" / "last_batch_block2_digests.npy"), r["digests"])
    assert np.array_equal(np.load(tmp_path / "a" / "last_batch_block2_container_pos.npy"), r["container_pos"])
    # a budget of 100 rows per block: a sorted, seeded sample of the rows, the same one every time
    monkeypatch.setattr(b, "DUMP_BUDGET", 3 * 100 * (3 * 8 + 4 * 21))
    b.dump_outputs(str(tmp_path / "c"), ctx, n_chunks, store, 0, 1)
    b.dump_outputs(str(tmp_path / "d"), ctx, n_chunks, store, 0, 1)
    o = np.load(tmp_path / "c" / "last_batch_block2_offsets.npy")
    assert len(o) == 100 and np.all(np.diff(o) >= 0) and np.isin(o, r["offsets"]).all()
    assert np.array_equal(o, np.load(tmp_path / "d" / "last_batch_block2_offsets.npy"))
    assert sum(os.path.getsize(tmp_path / "c" / f) for f in os.listdir(tmp_path / "c")) < 64 << 20
    # ranks of a node-global run write their own files
    b.dump_outputs(str(tmp_path / "e"), ctx, n_chunks, store, 1, 2)
    assert "n_chunks_rank1.npy" in os.listdir(tmp_path / "e") and "stats_rank1.npy" not in os.listdir(tmp_path / "e")


def test_fused_front_traffic_is_its_own(monkeypatch):
    """The fused front's PMC file is matched only when the line runs that front; the
    two-pass line keeps the two-pass file whatever sorts newest."""
    b = _bench(monkeypatch)
    d2, src2 = b.load_pmc(dict(WANT, workload="config2"))
    df, srcf = b.load_pmc(dict(WANT, workload="config2", front="fused"))
    assert src2 and srcf and src2 != srcf
    assert "lane_hash_kernel<5>" in df and "lane_hash_kernel<5>" not in d2
    assert "sha_carry_kernel<5>" in d2
