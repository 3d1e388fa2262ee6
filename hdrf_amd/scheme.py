"""ReductionScheme — the plugin API HDRF's README promises (README.md:3) and its DataNode hook
uses de facto:
  write: `new DataDeduplicator(ByteBuffer block, long blockId)` run by DDRunner
         (DN/DataDeduplicator.java:108, DN/DDRunner.java:20-36, DN/BlockReceiver.java:1258-1261)
  read:  `new DataConstructor(long blkID, byte[] recipe).data`   (DN/DataConstructor.java:46-73)
  length: FsDatasetImpl.getLength via Redis GET id               (DN/fsdataset/impl/FsDatasetImpl.java:736-763)

HipReductionScheme is the MI355X backend (libhdrf.so via ctypes; the Java DataNode binds the
same C-ABI through JNI).  Like DDRunner, `reduce` is one call per received
block in arrival order.
"""
import abc

from .lib import Context


class ReductionScheme(abc.ABC):
    """Abstract reduction scheme (one instance per DataNode)."""

    @abc.abstractmethod
    def reduce(self, block, block_id):
        """Reduce one received block (DataDeduplicator(ByteBuffer, long))."""

    @abc.abstractmethod
    def reconstruct(self, block_id):
        """Rebuild a block's bytes (DataConstructor(long, byte[]).data)."""

    @abc.abstractmethod
    def length(self, block_id):
        """Logical length of a reduced block (FsDatasetImpl.getLength for 0-byte replicas)."""


class HipReductionScheme(ReductionScheme):
    """GPU-backed scheme: `compressor` 1 (dedup) or 2 (dedup + Lz4Codec containers),
    DN/DataNode.java:438."""

    def __init__(self, hasher=0, device=0, compressor=1, **cfg):
        self.ctx = Context(hasher=hasher, compressor=compressor, device=device, **cfg)
        self.last = None

    def reduce(self, block, block_id):
        self.last = self.ctx.reduce_block(block, block_id)
        return self.last

    def reconstruct(self, block_id, verify=False):
        """verify=True: every chunk re-hashed against its recipe digest (HdrfError -8 on a mismatch)."""
        if verify:
            return self.ctx.reconstruct_block(block_id, verify=True).tobytes()
        return self.ctx.reconstruct_block(block_id).tobytes()

    def read(self, block_id, offset, length):
        """Bytes [offset, offset + length) of the block, clipped to its end (BlockSender's startOffset /
        length, DN/BlockSender.java:612-619): only the chunks under the range are gathered."""
        return self.ctx.read_range(block_id, offset, length).tobytes()

    read_range = read

    def prepare_reads(self, ids):
        """Build the seek tables of the stored blocks `ids`, so that ranged reads of them look up only the
        chunks under a range instead of the whole recipe.  Returns the per-id results (0 or an HDRF_E_*
        code).  A table lasts until its block is deleted, rewritten or the context is reset."""
        return self.ctx.seek_build(ids)

    def scrub(self, container=None):
        """Re-hash every stored chunk whose container is readable: (stats, bad chunks)."""
        return self.ctx.scrub(container)

    def length(self, block_id):
        return self.ctx.block_length(block_id)

    def delete(self, block_id):
        """Forget a block (FsDatasetImpl.invalidate); its chunks stay indexed until gc()."""
        self.ctx.block_delete(block_id)

    def gc(self, dry=False):
        """Drop every index entry no remaining recipe names: (stats, per-container rows)."""
        return self.ctx.gc(dry=dry)

    def compact(self, ids, dry=False, want_files=True):
        """Rewrite closed containers so that only the chunks the index still names remain:
        (per-container rows, {container id: its new chunkDir file})."""
        return self.ctx.compact(ids, dry=dry, want_files=want_files)

    def index_info(self):
        """The fingerprint table now: dict(index_log2, slots, entries, table_bytes)."""
        return self.ctx.index_info()

    def resize_index(self, new_log2):
        """Move the index into a table of 2^new_log2 slots while the scheme keeps running; a shrink that
        would load the table past 75 % is refused (HdrfError -4) and changes nothing."""
        self.ctx.index_resize(new_log2)

    def grow_index_if_loaded(self, threshold=0.6):
        """Grow the table by one bit when entries > threshold * slots (the write path slows past about
        60 % load).  Returns the new log2, or None when the table was left alone.  Nothing calls this
        implicitly: the DataNode decides when, e.g. after every few thousand blocks."""
        info = self.index_info()
        if info["entries"] <= threshold * info["slots"]:
            return None
        self.ctx.index_resize(info["index_log2"] + 1)
        return info["index_log2"] + 1

    def recipe(self, block_id):
        return self.ctx.recipe(block_id)

    def index_get(self, digest):
        return self.ctx.index_get(digest)

    def close(self):
        self.ctx.close()
