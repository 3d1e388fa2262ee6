"""bench.py as a process: a plain run times exactly --steps steps, runs none of the --full legs and,
with --dump-outputs, writes what the last timed step returned; --full on the same small corpus adds
the CPU legs and the whole-corpus check, whose verdict covers the dumped storeSizes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

# 8 blocks of 16 MiB in batches of 4: two batches per step, cross-batch duplicates
SMALL = ["--gpus", "1", "--blocks", "8", "--block-mib", "16", "--batch", "4", "--index-log2", "22",
         "--arena-slots", "128", "--steps", "3", "--warmup", "1"]


def _run(extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + SMALL + extra, cwd=ROOT,
                       env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    return json.loads(lines[0])


def test_plain_run_dumps_the_last_step_and_full_checks_it(tmp_path):
    out = tmp_path / "plain"
    line = _run(["--dump-outputs", str(out)])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["full"] is False
    assert line["ms_per_step"] > 0 and line["unit"] == "GB/s" and line["higher_is_better"] is True
    assert abs(line["value"] - 8 * (16 << 20) / (line["ms_per_step"] * 1e-3) / 1e9) <= 0.01 * line["value"]
    assert line["cpu_baseline"] is None and "configs" not in line and "oracle_check" not in line["dedup"]
    assert "alone" not in line["roofline"] and line["roofline"]["chains_ms_per_batch"]["W: chunking"] > 0
    files = sorted(os.listdir(out))
    assert sum(os.path.getsize(out / f) for f in files) <= 64 << 20
    arr = {f[:-4]: np.load(out / f) for f in files}
    assert all(a.dtype in (np.float32, np.float64) for a in arr.values())
    assert arr["n_chunks"].shape == (8,) and arr["n_chunks"].sum() == line["dedup"]["chunks"]
    assert arr["store_size"].sum() == line["dedup"]["stored_bytes"]
    for i in (0, 2, 3):                                   # first, middle and last block of the last batch (blocks 4, 6, 7)
        n = int(arr["n_chunks"][4 + i])
        assert arr["last_batch_block%d_offsets" % i].shape == (n,)
        assert arr["last_batch_block%d_offsets" % i][-1] == 16 << 20
        assert arr["last_batch_block%d_digests" % i].shape == (n, 20)
        new = arr["last_batch_block%d_is_new" % i]
        assert set(np.unique(new)) <= {0.0, 1.0} and new.shape == (n,)

    # the same arguments with --full: the same results (same inputs), now checked against the oracle
    out2 = tmp_path / "full"
    full = _run(["--full", "--no-sub", "--dump-outputs", str(out2)])
    assert full["full"] is True and "alone" in full["roofline"]
    assert sorted(os.listdir(out2)) == files
    for f in files:
        assert np.array_equal(np.load(out2 / f), arr[f[:-4]]), f
    chk = full["dedup"]["oracle_check"]
    assert chk["blocks"] == 8 and chk["store_size_mismatches"] == 0
    assert chk["stored_bytes_oracle"] == int(arr["store_size"].sum())
    cpu = full["cpu_baseline"]
    assert cpu["store_size_mismatches"] == 0 and cpu["chunk_check"]["mismatches"] == {"offsets": 0, "digests": 0, "is_new": 0}
