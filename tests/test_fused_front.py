"""HDRF_FUSED=1 in the environment changes nothing.  The variable once chose a fused chunk +
fingerprint front, which was removed; bench.py still reads it to pick the kernel
names it matches profiles against, so a process may carry it.  The library ignores it: a context
opened with it set gives the oracle's cuts, digests, decisions, containers and final state at the
edge sizes.  (The front's other tests left with it; tests/test_gpu_parity.py feeds their inputs.)"""
import pytest

from helpers import compare_block, compare_state, make_block
from hdrf_amd.lib import Context
from oracle.oracle import Oracle

pytestmark = pytest.mark.gpu

SMALL = dict(max_block_bytes=16 << 20, max_batch_blocks=8, index_log2=20, arena_slots=64)


@pytest.fixture
def fused(monkeypatch):
    monkeypatch.setenv("HDRF_FUSED", "1")


def run_sequence(blocks, hasher=0, container_max=1 << 25, compressor=1, **cfg):
    kw = dict(SMALL)
    kw.update(cfg)
    ctx = Context(hasher=hasher, container_max=container_max, compressor=compressor, **kw)
    ora = Oracle(hasher=hasher, compressor=compressor, max_size=container_max)
    ids = []
    for i, blk in enumerate(blocks):
        bid = 0x2000 + 5 * i
        compare_block(ctx.reduce_block(blk, bid), ora.reduce(blk, bid), tag=f"block {i}")
        ids.append(bid)
    compare_state(ctx, ora, ids)
    ctx.close()


@pytest.mark.parametrize("n", [0, 1, 700, 701, 702, 703, 1403, 4095, 65536 + 7])
def test_fused_edge_sizes(fused, n):
    run_sequence([make_block("random", n + 3, n), make_block("random", n + 3, n)])
