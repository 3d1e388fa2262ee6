/*
 * hdrf.h — C-ABI of libhdrf, the MI355X (gfx950) reduction backend for HDRF's
 * per-block write path (chunk -> fingerprint -> index -> container store).
 *
 * This is the drop-in boundary a DataNode binds through JNI.  Every
 * entry point replaces a piece of the reference's Java path; `DN/` abbreviates
 * hadoop-hdfs/src/main/java/org/apache/hadoop/hdfs/server/datanode/ in /root/reference.
 *
 * Conventions: plain pointers and sizes only; every function returns 0 on success or a
 * negative HDRF_E* code; hdrf_last_error() describes the last failure of a context; no C++
 * exception crosses this ABI.  A context is bound to one GPU.  Threads: every entry point takes
 * the context's lock, so any number of threads (one DataXceiver / DDRunner thread per block) may
 * call it concurrently (hdrf_close excepted: no call may be in progress or follow).  Block ORDER is
 * the call order unless the caller uses arrival tickets (hdrf_ticket_take at block arrival,
 * hdrf_reduce_block_ticketed later from any thread), which reproduce the reference's FIFO
 * (DN/DataDeduplicator.java:124-158, 197-204; DN/DDRunner.java:20-36).  hdrf_last_error() is the
 * context's last error, whichever thread caused it.
 */
#ifndef HDRF_H
#define HDRF_H
#include <stdint.h>
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

#define HDRF_OK 0
#define HDRF_E_INVAL (-1)      /* bad argument / configuration */
#define HDRF_E_HIP (-2)        /* HIP runtime failure */
#define HDRF_E_NOMEM (-3)      /* device or host allocation failed */
#define HDRF_E_CAPACITY (-4)   /* index table, arena or event list full */
#define HDRF_E_NOTFOUND (-5)   /* key / block / container absent */
#define HDRF_E_UNSUPPORTED (-6)/* option not implemented in this build */
#define HDRF_E_DEVICE (-7)     /* a kernel reported an inconsistency */
#define HDRF_E_CORRUPT (-8)    /* stored bytes do not hash to their fingerprint */

typedef struct hdrf_ctx hdrf_ctx;

/* Knobs of the reference, all compile-time statics there. */
typedef struct {
    int32_t hasher;          /* 0 SHA-1, 1 SHA-224          DataNode.hasher, DN/DataNode.java:446 */
    int32_t compressor;      /* 1 dedup, 2 dedup + Lz4Codec closed containers   DataNode.compressor :438 */
    int32_t window;          /* 700                         DataDeduplicator.chunking :266 */
    int32_t max_chunk;       /* 1000000                     DataDeduplicator.chunking :272 */
    int32_t n_thread;        /* 3                           DataDeduplicator.nThread :93 */
    int32_t min_mt_chunks;   /* 25                          DataDeduplicator :316, :514 */
    uint32_t container_max;  /* 2^25                        DataNode.maxSize :434 -> DataDeduplicator.maxSize */
    int32_t device;          /* HIP device ordinal */
    int64_t max_block_bytes; /* largest block (dfs.blocksize, 128 MiB) */
    int32_t max_batch_blocks;/* <= 64 blocks per hdrf_reduce_batch call */
    int32_t index_log2;      /* index table capacity = 2^index_log2 entries (64 B each) */
    int64_t arena_slots;     /* container arena slots of container_max bytes each */
    int32_t segment_bytes;   /* chunking speculation segment (default 1 MiB) */
    int32_t keep_recipes;    /* keep recipes (SET blockId -> size|digests) on the host */
    int32_t timing;          /* record per-stage HIP events */
    int32_t debug_tag_bits;  /* test hook (SHA-1 only): keep only this many index-tag bits to force
                                tag collisions through the exact slow path; 0 = full 64-bit tag */
    int32_t n_ranks;         /* GPUs sharing ONE node-global index (1 = this GPU is the whole node) */
    int32_t rank;            /* this GPU's rank in [0, n_ranks) = index partition it owns */
    int32_t retain_containers; /* 1: durable containers (a DataNode): a closed container keeps its arena
                                  slot until hdrf_drain_containers has handed it out, and a submit that
                                  could need such a slot returns HDRF_E_CAPACITY; 0 (default): the
                                  arena is a ring cache of the newest containers (benchmarks, tests) */
} hdrf_cfg;

/* Per-block result of hdrf_reduce_block (caller-owned host arrays; NULL to skip). */
typedef struct {
    int64_t n_chunks;        /* out */
    int64_t store_size;      /* out: bytes of new chunks (DataDeduplicator.storeSize :91,355) */
    int64_t capacity;        /* in: entries available in the arrays below */
    uint32_t *offsets;       /* chunk END offsets (DataDeduplicator.chunking :264-307) */
    uint8_t *digests;        /* n * H bytes (threadedHasher :578-641) */
    uint8_t *is_new;         /* chunkMeta.newChunk (DN/chunkMeta.java:35-60) */
    uint32_t *container_id;  /* new chunks: chunkMeta.blockID (:799) */
    uint32_t *container_pos; /* new chunks: chunkMeta.blockStart (:800) */
} hdrf_block_result;

int hdrf_default_cfg(hdrf_cfg *cfg);
/* DataNode.initializeDD (DN/DataNode.java:486-534) + JedisPool("localhost") (DN/DataDeduplicator.java:119) */
int hdrf_open(const hdrf_cfg *cfg, hdrf_ctx **out);
int hdrf_close(hdrf_ctx *ctx);
const char *hdrf_last_error(const hdrf_ctx *ctx);
int hdrf_digest_len(const hdrf_ctx *ctx);              /* DataNode.hash_length (:528-532) */

/* Write path, one block from host memory: replaces `new DataDeduplicator(bf1, blockId)`
 * launched by DDRunner (DN/DDRunner.java:26-36, DN/BlockReceiver.java:1258-1261).
 * Copies H2D, reduces, updates the index / containers / recipe / allocator. */
int hdrf_reduce_block(hdrf_ctx *ctx, uint64_t block_id, const uint8_t *data, uint64_t len,
                      hdrf_block_result *out);

/* Write path, a batch of device-resident blocks in arrival order (the FIFO order of
 * DN/DataDeduplicator.java:124-158).  data[i] must stay valid until the call returns and
 * provide readable[i] >= len[i] + 64 bytes.  Results of the batch stay on the device until
 * the next reduce call and are read with hdrf_batch_*. */
int hdrf_reduce_batch(hdrf_ctx *ctx, int32_t nblocks, const uint8_t *const *dev_data, const uint64_t *len,
                      const uint64_t *readable, const uint64_t *block_ids);

/* Pipelined form of hdrf_reduce_batch: hdrf_submit_batch enqueues the batch (chunking, SHA and
 * index + store on three HIP streams, in block order; under compressor 2 the batch's LZ4 pass runs
 * on one of two LZ4 streams, so consecutive batches' passes overlap) and returns; hdrf_wait_batch
 * completes the
 * OLDEST submitted batch and makes it the one hdrf_batch_* report.  At most HDRF_PIPELINE_DEPTH
 * batches are in flight: a submit beyond that returns HDRF_E_CAPACITY (call hdrf_wait_batch
 * first), so every submit pairs with exactly one wait.  The device buffers of a batch must stay
 * valid until it is completed.  Chunking of batch k+1 overlaps hashing of batch k and the
 * index/store stage of batch k-1 (latency-bound walk, VALU-bound SHA, HBM-bound store); the
 * bench keeps three batches in flight (five under compressor 2, where a batch's LZ4 pass outlasts
 * the front halves of the next ones).  Views (index, containers, allocator) complete all batches
 * first. */
#define HDRF_PIPELINE_DEPTH 5
int hdrf_submit_batch(hdrf_ctx *ctx, int32_t nblocks, const uint8_t *const *dev_data, const uint64_t *len,
                      const uint64_t *readable, const uint64_t *block_ids);
int hdrf_wait_batch(hdrf_ctx *ctx);
/* The streaming DataNode write path (BASELINE config 5; the hook's bf1 handed over at
 * DN/BlockReceiver.java:1258-1261): host-resident blocks are copied H2D on a side stream
 * (hipMemcpyAsync from pinned memory overlaps the kernels of the batches in flight) into the
 * batch slot's staging buffer, then reduced exactly as hdrf_submit_batch.  The host buffers must
 * stay valid and unmodified until the batch completes (hdrf_wait_batch).  No 16-B alignment or
 * slack is required of host buffers. */
int hdrf_submit_host(hdrf_ctx *ctx, int32_t nblocks, const uint8_t *const *host_data, const uint64_t *len,
                     const uint64_t *block_ids);
/* Packet-granular receive (DN/BlockReceiver.java:877-896, 1258-1261): hdrf_rx_begin reserves one of
 * 16 device receive buffers for a block (blocks received concurrently, as a DataNode runs one
 * DataXceiver per block being written); hdrf_append_packet copies each packet as it arrives into the
 * buffer's own pair of pinned 4 MiB staging chunks (the packet may be reused when the call returns)
 * and sends every full chunk H2D on a side stream, overlapped with the next packets and with the
 * blocks in flight.  The packets of one receive buffer come from one thread at a time (the block's
 * receiver); hdrf_append_packet does not take the context lock, so receivers of different blocks
 * copy concurrently;
 * hdrf_submit_slot submits the received block as a one-block batch with no copy left (pair it
 * with hdrf_wait_batch like hdrf_submit_batch; HDRF_E_CAPACITY when the pipeline is full).  The
 * buffer is free again when that batch completes; hdrf_rx_begin returns HDRF_E_CAPACITY while all
 * sixteen are in use.  hdrf_rx_cancel gives back a buffer whose block is abandoned (the client was
 * lost mid-block; the reference drops bf1): its receiver must have stopped appending.  A packet
 * that would take the block past max_block_bytes is refused (HDRF_E_INVAL) and copies nothing.
 * hdrf_reset refuses (HDRF_E_INVAL) while a buffer is receiving; hdrf_close requires every
 * receiver to have stopped.  hdrf_submit_slots submits n <= max_batch_blocks received blocks
 * (receive buffers listed in arrival order) as ONE batch: a DataNode whose receivers finished several
 * blocks since its last submit hands them over together (the FIFO order is the list order), so the
 * per-batch index / store passes are shared; the buffers are free again when that batch completes. */
int hdrf_rx_begin(hdrf_ctx *ctx, uint64_t block_id, int32_t *rx);
int hdrf_append_packet(hdrf_ctx *ctx, int32_t rx, const uint8_t *data, uint64_t len);
int hdrf_submit_slot(hdrf_ctx *ctx, int32_t rx);
int hdrf_submit_slots(hdrf_ctx *ctx, int32_t n, const int32_t *rx);
int hdrf_rx_cancel(hdrf_ctx *ctx, int32_t rx);
/* Stream-mode schemes (DataNode.compressor 0/3/4/5: the whole block through a Hadoop codec,
 * DN/BlockReceiver.java:822-894,1238-1256).  codec 4 = Lz4Codec, 0 = SnappyCodec, 3 = LzopCodec
 * (hadoop-lzo: LZO1X-1 blocks in an lzop file; the header's mtime is hdrf_set_lzop_mtime's value,
 * default 0, where the reference writes the wall clock), 5 = GzipCodec: the file
 * the reference writes to chunkDir+id when the block arrives as write()s of the given sizes (one
 * per packet, summing to len) followed by close().  dev_data needs len + 64 readable bytes.
 * Returns the file length (written to out), HDRF_E_CAPACITY if cap is too small,
 * HDRF_E_UNSUPPORTED for other codecs.  Codec 5's file does not depend on the write sizes
 * (zlib level 6 fed through Hadoop's ZlibCompressor); they must still add up to len.
 * Records the block length (SET id -> BE32(len)) for hdrf_block_length. */
int64_t hdrf_stream_block(hdrf_ctx *ctx, int32_t codec, uint64_t block_id, const uint8_t *dev_data, uint64_t len,
                          uint64_t readable, const uint64_t *writes, int32_t nwrites, uint8_t *out, int64_t cap);
/* hdrf_stream_block for a host-resident block (copied H2D first; no alignment or slack needed). */
int64_t hdrf_stream_block_host(hdrf_ctx *ctx, int32_t codec, uint64_t block_id, const uint8_t *data, uint64_t len,
                               const uint64_t *writes, int32_t nwrites, uint8_t *out, int64_t cap);
/* Read side for container / block FILES (DataConstructor's Lz4Codec input stream,
 * DN/DataConstructor.java:171-176,495-500): hdrf_lz4_file_decode decodes a Hadoop Lz4Codec file
 * (BlockCompressorStream framing, as written by compressor 2 containers and compressor 4 blocks)
 * on the GPU into dev_out; returns the raw length (HDRF_E_INVAL on a malformed file).
 * hdrf_container_load makes container `id` readable for hdrf_reconstruct* again from its chunkDir
 * file (lz4 = 1 for a closed container's Lz4Codec file, 0 for raw bytes) after its arena slot was
 * reused or the DataNode restarted; hdrf_container_unload frees that copy. */
int64_t hdrf_lz4_file_decode(hdrf_ctx *ctx, const uint8_t *file, int64_t flen, uint8_t *dev_out, int64_t cap);
/* The same for a stream-mode block file of codec 0 (SnappyCodec), 3 (LzopCodec: lzop header and
 * its checksum checked, LZO1X blocks decoded on the GPU), 4 (Lz4Codec) or 5 (GzipCodec:
 * gzip members, inflated on the GPU, CRC-32 and ISIZE checked): the compression-only decoders of
 * DataConstructor (DN/DataConstructor.java:102-220).  HDRF_E_INVAL on a malformed file. */
int64_t hdrf_stream_file_decode(hdrf_ctx *ctx, int32_t codec, const uint8_t *file, int64_t flen, uint8_t *dev_out,
                                int64_t cap);
/* The mtime field of the lzop headers hdrf_stream_block writes for codec 3 (LzopOutputStream puts
 * System.currentTimeMillis() / 1000 there, the only bytes of the file that are not a function of
 * the block). */
int hdrf_set_lzop_mtime(hdrf_ctx *ctx, uint32_t mtime);
/* Stage 1 of the GPU compressor 5 (GzipCodec = zlib level 6 deflate_slow, DN/BlockReceiver.java:
 * 858-873): for every position p of the len device bytes, the answer zlib's
 * longest_match gives at p with a 128-candidate chain (out128, prev_length < 8) and a 32-candidate
 * chain (out32, prev_length 8..15): (len << 16) | distance, 0 when no match of >= 3 bytes, bit 31
 * when the head candidate is a window-base position at distance exactly MAX_DIST.  dev_prev is
 * len u32 of scratch (the hash-chain predecessor + 1).  Synchronous on the context's stream. */
int hdrf_gzip_match_pass(hdrf_ctx *ctx, const uint8_t *dev_data, uint64_t len, uint32_t *dev_prev,
                         uint32_t *dev_out128, uint32_t *dev_out32);
/* Stage 2 of the GPU compressor 5: zlib's lazy parse (deflate_slow) over stage 1's answers.
 * dev_syms (len + 1 u32) receives (dist << 8) | lc per symbol (dist 0: literal lc; else lc =
 * length - 3); dev_blks (5 * (len / 16383 + 2) int64) one row per deflate block (symbol end,
 * block_start, strstart, window base, last); dev_cnt (2 int64) = {symbols, blocks}. */
int hdrf_gzip_parse(hdrf_ctx *ctx, const uint8_t *dev_data, uint64_t len, const uint32_t *dev_m128,
                    const uint32_t *dev_m32, uint32_t *dev_syms, int64_t *dev_blks, int64_t *dev_cnt);
int hdrf_container_load(hdrf_ctx *ctx, uint32_t id, const uint8_t *file, int64_t flen, int32_t lz4);
int hdrf_container_unload(hdrf_ctx *ctx, uint32_t id);
/* Restore a DataNode from its persisted state (the Redis keys + chunkDir files), on a fresh or
 * reset context: hdrf_index_load SETs digest -> 11-B value for n rows (keys n*H bytes, vals n*11,
 * e.g. the output of hdrf_index_dump); hdrf_allocator_load SETs "blockID" (24 B, as returned by
 * hdrf_allocator) and reopens each storer range's open container from its file (open_len[t] < 0:
 * no file); hdrf_recipe_load SETs longToBytes(id,4) -> recipe.  Blocks reduced afterwards, and
 * their containers, are those of a DataNode that never stopped. */
int hdrf_index_load(hdrf_ctx *ctx, const uint8_t *keys, const uint8_t *vals, int64_t n);
int hdrf_allocator_load(hdrf_ctx *ctx, const uint8_t alloc24[24], const uint8_t *const *open_files,
                        const int64_t *open_len);
int hdrf_recipe_load(hdrf_ctx *ctx, uint64_t block_id, const uint8_t *recipe, int64_t len);
/* Pinned (page-locked) host memory for hdrf_submit_host buffers. */
int hdrf_host_alloc(hdrf_ctx *ctx, uint64_t bytes, void **out);
int hdrf_host_free(hdrf_ctx *ctx, void *p);
/* Number of blocks of the batch hdrf_batch_* report (the last completed one). */
int hdrf_batch_nblocks(hdrf_ctx *ctx);

int hdrf_batch_info(hdrf_ctx *ctx, int32_t b, int64_t *n_chunks, int64_t *store_size);
int hdrf_batch_offsets(hdrf_ctx *ctx, int32_t b, uint32_t *out, int64_t cap);
int hdrf_batch_digests(hdrf_ctx *ctx, int32_t b, uint8_t *out, int64_t cap_bytes);
int hdrf_batch_is_new(hdrf_ctx *ctx, int32_t b, uint8_t *out, int64_t cap);
int hdrf_batch_placement(hdrf_ctx *ctx, int32_t b, uint32_t *cid, uint32_t *pos, int64_t cap);
/* Test hook (in the spirit of debug_tag_bits): which way the chunker's bookkeeping went for block b of
 * the batch hdrf_batch_* report.  One record per lane-walk segment of the block, in order: the
 * speculative walk's main / overrun cut counts, the boundary's final status (sync >= 0: overrun cut
 * sync & 0xffff equals the next segment's cut sync >> 16; -1 the chain ran to the block end; -3
 * repaired: it met segment + jmp at that segment's cut jj after n_ext repair cuts; -4 the repair gave
 * up), where the repair's cuts went in the block's offsets (ext_dst, -1: the boundary is not on the
 * block's path) and how many offsets the segment contributed (n_piece, 0 off the path).
 * *rq_count = the batch's failed speculative boundaries (the repair queue's length), all blocks.
 * Returns the block's segment count (HDRF_E_CAPACITY when cap is smaller).  Read-only: it copies
 * what the batch's chunking kernels left in the pipeline slot and launches nothing.  Validity: like
 * hdrf_batch_offsets, from the hdrf_wait_batch (or hdrf_reduce_*) that completed the batch until the
 * slot is submitted to again, i.e. until HDRF_PIPELINE_DEPTH - 1 further batches have been submitted;
 * a submit waits for its slot's previous batch, so nothing in flight writes the slot in between.
 * Single-GPU contexts only (n_ranks = 1). */
typedef struct {
    int32_t n_main, n_over, sync, jmp, jj, n_ext, ext_dst, n_piece;
} hdrf_seg_trace;
int hdrf_batch_seg_trace(hdrf_ctx *ctx, int32_t b, hdrf_seg_trace *out, int64_t cap, int32_t *rq_count);

/* Index (Redis) views. GET digest -> 11-byte chunkMeta value (DN/chunkMeta.java:62-77).
 * Returns 1 if found, 0 if absent, <0 on error. */
int hdrf_index_get(hdrf_ctx *ctx, const uint8_t *digest, uint8_t out11[11]);
int64_t hdrf_index_count(hdrf_ctx *ctx);
/* Probe lengths of the last completed batch: each chunk's distance (entries) from its home slot to
 * the entry its digest resolved to (linear probing); sum, max and chunk count.  Measurement only.
 * After hdrf_index_resize the batch's slots are those of the old table: all three are 0 until a batch
 * has completed in the new one. */
int hdrf_probe_stats(hdrf_ctx *ctx, int64_t *probe_sum, int64_t *probe_max, int64_t *chunks);
/* All (digest, value) pairs sorted by digest; returns count (or HDRF_E_CAPACITY). */
int64_t hdrf_index_dump(hdrf_ctx *ctx, uint8_t *keys, uint8_t *vals, int64_t cap);
/* GET "blockID": 24-byte allocator (utilities.blockIDtoBytes, DN/utilities.java:66-75).
 * Returns 1 if the key exists (a block was reduced), 0 otherwise. */
int hdrf_allocator(hdrf_ctx *ctx, uint8_t out24[24]);
/* GET longToBytes(blockId,4): recipe [BE32 size | digests] (DataDeduplicator.storeDB :372-392).
 * Returns length, 0 if absent; HDRF_E_CAPACITY if cap is too small (needs keep_recipes). */
int64_t hdrf_recipe_get(hdrf_ctx *ctx, uint64_t block_id, uint8_t *out, int64_t cap);
/* FsDatasetImpl.getLength for 0-byte replicas (DN/fsdataset/impl/FsDatasetImpl.java:736-763). */
int64_t hdrf_block_length(hdrf_ctx *ctx, uint64_t block_id);
/* Container file chunkDir+id as it is now (the batches in flight complete first).  Returns length;
 * *closed = 1 once it overflowed.  Raw bytes, except closed containers under compressor 2: the
 * Lz4Codec file the storer rewrote (:770-779).  HDRF_E_NOTFOUND if it never existed or its arena
 * slot was recycled (cfg.retain_containers = 0), or after a drain handed it out and its slot was
 * reused (retain_containers = 1: the file is the caller's then). */
int64_t hdrf_container_read(hdrf_ctx *ctx, uint32_t id, uint8_t *out, int64_t cap, int32_t *closed);

/* Durable containers (cfg.retain_containers = 1): what the storers wrote to chunkDir since the
 * last drain (DN/DataDeduplicator.java:748-818).  Each event is one file operation:
 *   closed = 1   the container closed (:748-786): write nbytes bytes at file_off of chunkDir+id and
 *                the file is final.  Under compressor 2 file_off = 0 and the bytes are the whole
 *                Lz4Codec file (rewrite it).  Under compressor 1 the storer's rewrite (prevData ||
 *                buffer) leaves the bytes already handed out in place, so only the rest travels:
 *                file_off = the file's length so far (0 when nothing was handed out yet)
 *   closed = 0   the open container grew: write nbytes bytes at file_off (= the file's length so
 *                far) of chunkDir+id, creating it when file_off == 0 (:806-818)
 * The bytes of event i are out[data_off, data_off + nbytes).  Events come in order (closes in
 * close order, then the open containers) and whole; returns the number written, 0 when nothing is
 * pending, HDRF_E_CAPACITY (and *need = the next event's bytes) when not even one fits.  Call again
 * until it returns 0.  Hands out what the COMPLETED batches (hdrf_wait_batch) produced; batches
 * still in flight keep running (their containers come with a later drain), so a DataNode drains
 * after every hdrf_wait_batch without stalling the pipeline.  The copies run on a stream of their
 * own, beside the H2D copies of later blocks.  A drained closed container's slot may then be
 * reused; read it back with hdrf_container_load. */
typedef struct {
    uint32_t id;             /* container id (utilities.bytesToBlockID ranges, DN/utilities.java:36-75) */
    int32_t closed;
    int64_t file_off;
    int64_t nbytes;
    int64_t data_off;
} hdrf_container_event;
int64_t hdrf_drain_containers(hdrf_ctx *ctx, hdrf_container_event *ev, int64_t ev_cap, uint8_t *out, int64_t out_cap,
                              int64_t *need);

/* Arrival tickets (AIWriteQueue, DN/DataDeduplicator.java:124-158): take one when a block arrives
 * (BlockReceiver, before its DDRunner starts), reduce with it from any thread: a ticketed call waits
 * until every earlier ticket has been reduced or cancelled, so the index / containers / recipes
 * are those of the arrival order.  A ticket that will never be used must be cancelled. */
int hdrf_ticket_take(hdrf_ctx *ctx, uint64_t *ticket);
int hdrf_ticket_cancel(hdrf_ctx *ctx, uint64_t ticket);
int hdrf_reduce_block_ticketed(hdrf_ctx *ctx, uint64_t ticket, uint64_t block_id, const uint8_t *data, uint64_t len,
                               hdrf_block_result *out);

/* Read side: DataConstructor(blkID, recipe).data (DN/DataConstructor.java:73-250, 360-531), the
 * rebuild BlockSender serves on READ_BLOCK (DN/BlockSender.java:612-619).  Every recipe digest
 * is looked up in the index; its chunk, container[start, stop), lands at the running sum of the
 * chunk lengths.  hdrf_reconstruct writes to device memory and returns the block size;
 * hdrf_reconstruct_block uses the context's stored recipe and copies to host memory.  The
 * containers must still be resident (HDRF_E_NOTFOUND otherwise).  Single-node contexts. */
int64_t hdrf_reconstruct(hdrf_ctx *ctx, const uint8_t *recipe, int64_t recipe_len, uint8_t *dev_out, int64_t cap);
int64_t hdrf_reconstruct_block(hdrf_ctx *ctx, uint64_t block_id, uint8_t *out, int64_t cap);

/* Fingerprint scrub and verified reads.  The store is content-addressed: every chunk's index key is
 * the SHA-1 / SHA-224 of its bytes, so stored bytes can be checked against the key that names them
 * (what the DataNode block scanner and the checksums of an HDFS read do for block files). */
typedef struct {
    uint8_t  digest[28];        /* the index key (first digest_len bytes) */
    uint32_t container, start, stop;
    int32_t  why;               /* 1: bytes hash to another digest; 2: [start, stop) not inside the container's bytes */
} hdrf_bad_chunk;

typedef struct {
    int64_t entries;            /* live index entries seen (after the container filter) */
    int64_t checked;            /* hashed and compared */
    int64_t skipped;            /* container neither arena-resident nor loaded */
    int64_t bytes;              /* bytes hashed */
    int64_t bad;                /* == the return value */
} hdrf_scrub_stats;

/* Scrub: every index entry whose container is readable (arena-resident, or loaded with
 * hdrf_container_load) is re-hashed from the container's bytes and compared with its key.
 * container = -1: all readable containers; otherwise that id (HDRF_E_NOTFOUND if not readable).
 * Returns the number of bad chunks; the first min(bad, cap) are written sorted by
 * (container, start, digest).  A view: completes the batches in flight first.  Single-node contexts. */
int64_t hdrf_scrub(hdrf_ctx *ctx, int64_t container, hdrf_bad_chunk *bad, int64_t cap, hdrf_scrub_stats *st);

/* hdrf_reconstruct / hdrf_reconstruct_block, then every chunk of the rebuilt block re-hashed and
 * compared with its recipe digest.  Returns the block size, or HDRF_E_CORRUPT with *bad_chunk = the
 * lowest recipe position that failed (the block's bytes are in the output anyway; hdrf_last_error
 * names the digest, the container and the range).  *bad_chunk = -1 otherwise. */
int64_t hdrf_reconstruct_verified(hdrf_ctx *ctx, const uint8_t *recipe, int64_t recipe_len, uint8_t *dev_out,
                                  int64_t cap, int64_t *bad_chunk);
int64_t hdrf_reconstruct_block_verified(hdrf_ctx *ctx, uint64_t block_id, uint8_t *out, int64_t cap, int64_t *bad_chunk);

/* Batched, ranged reads.  An HDFS read names a byte range: BlockSender is built with startOffset and
 * length, and the reference rebuilds the whole block and seeks into it (DN/BlockSender.java:612-619:
 * new DataConstructor(id, t1data), then new ByteArrayInputStream(dConstructor.data, (int) offset, ...)).
 * hdrf_read_batch serves n <= HDRF_READ_MAX_REQS requests, each one byte range of one block, with one
 * set of launches and one host wait; only the chunks that overlap a range are copied.
 *   When it runs   a view: it completes the batches in flight and applies a pending hdrf_reset_async,
 *                  as hdrf_reconstruct does, and takes the context lock.  Single-node contexts
 *                  (HDRF_E_UNSUPPORTED when n_ranks > 1).
 *   Ranges         offset > size: that request gets HDRF_E_INVAL.  offset == size or length == 0: 0
 *                  bytes.  A length past the block's end is clipped to size - offset.
 *   Outputs        a request that succeeds writes exactly [dev_out, dev_out + result): no byte before
 *                  or after that span is touched.  A request that fails writes nothing (never a partial
 *                  block, per request).  The output ranges of different requests must not overlap (the
 *                  result is undefined if they do).
 *   Failures       one failing request does not stop the others: every req[i].result is filled; the
 *                  call returns 0 when every request succeeded, otherwise the code of the
 *                  lowest-numbered failing request, which hdrf_last_error names.  Call-level failures
 *                  (NULL arguments, n outside [0, HDRF_READ_MAX_REQS], allocation or HIP failure)
 *                  return their code and touch no output.
 *   HDRF_E_NOTFOUND  there is no recipe for block_id; or a recipe digest is absent from the index,
 *                  wherever it sits in the recipe (the offsets cannot be computed without it); or a
 *                  chunk that overlaps the requested range sits in a container that is not readable
 *                  (chunks outside the range may: a ranged read needs only the containers it touches).
 *   HDRF_E_DEVICE  the chunk lengths of the recipe do not add up to its BE32 size.
 * hdrf_read_range is one request through the same path for a stored recipe, with the clipped range
 * copied to host memory (only those bytes travel); HDRF_E_CAPACITY when cap is below the clipped
 * length.  Returns the bytes written. */
#define HDRF_READ_MAX_REQS 256
typedef struct {
    uint64_t block_id;       /* recipe from the context's store (keep_recipes / hdrf_recipe_load) ... */
    const uint8_t *recipe;   /* ... unless non-NULL: [BE32 size | digests], host memory, as hdrf_reconstruct takes */
    int64_t  recipe_len;
    uint64_t offset;         /* first byte wanted (BlockSender's startOffset) */
    uint64_t length;         /* bytes wanted; clipped to size - offset */
    uint8_t *dev_out;        /* device memory, any alignment, `clipped length` bytes, no slack needed */
    int64_t  result;         /* out: bytes written (the clipped length), or a negative HDRF_E_* */
} hdrf_read_req;
int hdrf_read_batch(hdrf_ctx *ctx, int32_t n, hdrf_read_req *req);
int64_t hdrf_read_range(hdrf_ctx *ctx, uint64_t block_id, uint64_t offset, uint64_t length, uint8_t *out, int64_t cap);

/* Seek tables.  Without one, a ranged read looks up EVERY digest of the block's recipe: a chunk's offset
 * in the block is the sum of all earlier chunk lengths, and those live only in the index entries.  The
 * seek table of a stored recipe of n chunks is end[0..n), u32: end[k] is the block offset one past chunk
 * k.  The tables live in a device store of their own, beside the recipe store.
 * hdrf_seek_build builds (or rebuilds) the tables of n >= 0 blocks:
 *   When it runs   a view: it takes the context lock and completes the batches in flight, as
 *                  hdrf_read_batch does.  Single-node contexts (HDRF_E_UNSUPPORTED when n_ranks > 1).
 *   What it does   for every id it looks up every digest of the stored recipe, adds up the lengths and
 *                  checks the total against the recipe size.  Only the index is needed: no container has
 *                  to be readable.  The ids are worked through in groups, so the scratch stays bounded
 *                  whatever n is.
 *   Failures       per id, in result[i] (result may be NULL): HDRF_E_NOTFOUND when there is no stored
 *                  recipe (which includes cfg.keep_recipes == 0) or a digest is absent from the index,
 *                  HDRF_E_DEVICE when the lengths do not add up to the size.  A failed id keeps no table
 *                  (an older table of it is dropped).  One failure does not stop the others; the call
 *                  returns the code of the lowest-numbered failing id, 0 when there is none.  Call-level
 *                  failures: HDRF_E_INVAL (NULL context, n < 0, n > 0 without ids), HDRF_E_NOMEM,
 *                  HDRF_E_CAPACITY (a recipe of more than 2^24 chunks), HDRF_E_HIP.
 *   Lifetime       a table goes away, without a launch, with hdrf_block_delete of its block, with any new
 *                  recipe for its id (a write or hdrf_recipe_load), with hdrf_reset (and an
 *                  hdrf_reset_async when it is applied), hdrf_seek_drop and hdrf_close.  It stays valid
 *                  through hdrf_gc (a live recipe's digests are kept), hdrf_compact (start and stop
 *                  move, lengths do not) and hdrf_index_resize (entries move verbatim).
 * hdrf_seek_drop forgets the tables of n ids (unknown ids are ignored); ids == NULL: all of them, and the
 * store's memory is freed (dropped tables' bytes are not reclaimed one by one: drop all and build again).
 * hdrf_seek_info_get: what the store holds and what the last hdrf_read_batch* / hdrf_read_range* call did.
 *
 * With a table hdrf_read_batch and hdrf_read_range serve a request that names a stored recipe by
 * block_id from it; a request that carries its own recipe, or whose block has no table, goes the way
 * described above, and one call may mix both.  The contract above holds, and in addition:
 *   - only the digests and the containers of the chunks under the range are consulted: a digest absent
 *     from the index elsewhere in the recipe, or an unreadable container there, does not fail the request;
 *   - a zero-length request (length == 0 or offset == size) returns 0 without a lookup;
 *   - HDRF_E_DEVICE also tells that the table and the index disagree on the length of a chunk under the
 *     range (hdrf_last_error says so).  No public call produces that state deterministically (loading
 *     a digest that is present is outside hdrf_index_load's contract): the check is a guard;
 *   - last_rows counts the chunk rows the call's lookups ran over: the whole recipe for a request without
 *     a table, min(n, clipped length / max(minlen, 1) + 2) for one with a table and a non-empty range,
 *     where minlen is the smallest length among the recipe's chunks but the last (the chunks strictly
 *     inside a range are that long at least, and two more are cut by its ends); last_seek_reqs counts
 *     the requests served from a table. */
typedef struct {
    int64_t blocks;          /* tables held */
    int64_t chunks;          /* ... and the chunks they describe */
    int64_t bytes;           /* device bytes of the seek store (allocated, whether or not a table uses them) */
    int64_t last_rows;       /* the last read call: chunk rows its lookups ran over */
    int64_t last_seek_reqs;  /* ... and requests served from a table */
} hdrf_seek_info;
int hdrf_seek_build(hdrf_ctx *ctx, const uint64_t *block_ids, int32_t n, int32_t *result);
int hdrf_seek_drop(hdrf_ctx *ctx, const uint64_t *block_ids, int32_t n);
int hdrf_seek_info_get(hdrf_ctx *ctx, hdrf_seek_info *out);

/* Verified ranged reads: hdrf_read_batch / hdrf_read_range as above (with or without a seek table), then,
 * on the same stream, every chunk that shares a byte with a successful request's range is re-hashed WHOLE
 * and compared with its recipe digest.  A chunk that lies wholly inside the range is hashed from the
 * output bytes, which checks the gather as well as the container; the at most two chunks the range cuts
 * are hashed from their container's bytes (the copy of their served part is not covered).  On a mismatch
 * the request's result is HDRF_E_CORRUPT and bad_chunk[i] is the lowest failing position IN THE RECIPE
 * (not in the range); the range's bytes are in the output anyway, and hdrf_last_error names the digest,
 * the container and the range of the first such request.  bad_chunk[i] = -1 otherwise (n entries;
 * hdrf_read_range_verified: one).  HDRF_E_INVAL when bad_chunk is NULL. */
int hdrf_read_batch_verified(hdrf_ctx *ctx, int32_t n, hdrf_read_req *req, int64_t *bad_chunk);
int64_t hdrf_read_range_verified(hdrf_ctx *ctx, uint64_t block_id, uint64_t offset, uint64_t length, uint8_t *out,
                                 int64_t cap, int64_t *bad_chunk);

/* The same read on a node-global context (cfg.n_ranks = G > 1): the node's ONE index is
 * partitioned over the ranks, and a container's bytes are spread over the ranks that placed
 * chunks into it, so every rank takes part (hdrf_amd/node.py NodeRank.reconstruct_block; the
 * shared Redis of DN/DataConstructor.java:360-417 serves any DataNode):
 *   1. every rank gets the block's n recipe digests (n * digest_len bytes, host);
 *      hdrf_gx_read_locate fills loc[4k..4k+3] = {container id, start, stop, placing rank + 1}
 *      for the digests it owns (first digest word mod G == rank) and zeros for the others;
 *      returns how many it owns, HDRF_E_NOTFOUND if an owned digest is absent;
 *   2. the G loc arrays are summed (the rows are disjoint);
 *   3. hdrf_gx_read_fill writes, at each chunk's block offset (running sum of stop - start) of
 *      dev_out (zeroed by the caller), the chunks this rank placed; returns the bytes written
 *      (HDRF_E_NOTFOUND when such a chunk's container left the arena ring);
 *   4. the G partial blocks summed byte-wise (disjoint) on the reading rank are the block; the
 *      returned counts sum to the recipe size.
 * Call between batches (no hdrf_gx_* batch in flight); both first complete the last batch's commit
 * and arena copy on this rank (as hdrf_gx_sync, whose commit error they report). */
int64_t hdrf_gx_read_locate(hdrf_ctx *ctx, const uint8_t *digests, int64_t n, uint32_t *loc);
int64_t hdrf_gx_read_fill(hdrf_ctx *ctx, const uint32_t *loc, int64_t n, uint8_t *dev_out, int64_t cap);

/* Block deletion and index garbage collection.  HDFS deletes blocks all the time: BPOfferService calls
 * FsDatasetImpl.invalidate (DN/fsdataset/impl/FsDatasetImpl.java:2026-2100), which in the reference
 * removes the 0-byte block file and its .meta and leaves the recipe, the chunks' index entries and the
 * container bytes behind forever.
 * hdrf_block_delete forgets a block: it completes the batches in flight (as the views do), then drops
 * the block's recipe location and its length (so stream-mode blocks are covered too) and subtracts the
 * recipe from hdrf_stats.recipe_bytes.  HDRF_E_NOTFOUND for a block the context does not know.
 * Afterwards hdrf_recipe_get returns 0 and hdrf_block_length, hdrf_reconstruct_block* and hdrf_read_range
 * return HDRF_E_NOTFOUND.  The index is not touched (the delete is cheap; collection happens later), and
 * the recipe's bytes in the append-only device recipe store are not reclaimed: compacting that store is
 * out of scope.
 * hdrf_gc collects the index: the live set is the set of digests of all recipes the context holds; an
 * index entry whose digest is in it is kept, every other live entry is dropped.
 *   When it runs   it takes the context lock, completes the batches in flight and applies a pending
 *                  hdrf_reset_async, like the other views and restores.  Single-node contexts
 *                  (HDRF_E_UNSUPPORTED when n_ranks > 1).  HDRF_E_INVAL when cfg.keep_recipes == 0 (the
 *                  context's recipes are then not the complete live set, and collecting would drop
 *                  live chunks) and while a packet receive is open, as hdrf_reset.
 *   Returns        the number of container rows: one for every container id that some index entry
 *                  named before the collection; the first min(rows, cap) are written sorted by id.
 *                  A container with kept_chunks == 0 is dead: the DataNode may delete its chunkDir
 *                  file once it is closed.  A recipe digest absent from the index is counted in
 *                  `missing` (once per occurrence in a recipe) and is no error.  GC frees no arena slot and unloads nothing: the arena
 *                  stays the ring or retained store that it is, and the bytes of the dropped chunks of
 *                  a container that keeps others stay in its file.
 *   Changes        with HDRF_GC_DRY nothing.  Otherwise the index afterwards holds exactly the kept
 *                  entries, their 11-byte values unchanged; a dropped digest is absent (hdrf_index_get
 *                  returns 0), and a later write of those bytes stores them as new chunks, exactly as
 *                  on a DataNode that never saw them.  The index is rebuilt from the kept entries
 *                  under a new table epoch; any failure before that switch (allocation, a counter
 *                  check) leaves the index exactly as it was, a failure after it returns
 *                  HDRF_E_DEVICE / HDRF_E_HIP and marks the context for hdrf_reset. */
#define HDRF_GC_DRY 1          /* mark and account only; the index is not touched */
typedef struct {
    int64_t recipes, recipe_digests;     /* live recipes walked, digests looked up */
    int64_t entries;                     /* live index entries before the collection */
    int64_t kept, dropped;               /* entries == kept + dropped */
    int64_t kept_bytes, dropped_bytes;   /* sum of stop - start over each */
    int64_t missing;                     /* recipe digests absent from the index (reported, not an error) */
    int64_t containers, dead_containers; /* containers named by an entry before / with no kept entry */
} hdrf_gc_stats;
typedef struct {
    uint32_t id; int32_t readable;       /* 1: arena-resident or loaded */
    int64_t kept_chunks, kept_bytes, dropped_chunks, dropped_bytes;
} hdrf_gc_container;
/* FsDatasetImpl.invalidate: forget a block. */
int hdrf_block_delete(hdrf_ctx *ctx, uint64_t block_id);
int64_t hdrf_gc(hdrf_ctx *ctx, int32_t flags, hdrf_gc_stats *st, hdrf_gc_container *rows, int64_t cap);

/* Container compaction: give back the bytes of dropped chunks.  hdrf_gc drops index entries and
 * reports, per container, the bytes nobody names any more (dropped_bytes); a container's chunkDir file
 * can only be deleted when nothing in it is kept.  hdrf_compact rewrites the closed containers the
 * caller names so that only the chunks live index entries name remain, packed to the front in their
 * old order: sort the container's live entries by start; chunk k's new start is the sum of the lengths
 * of chunks 0..k-1, its new stop is start + length, its bytes are copied unchanged.
 *   When it runs   it takes the context lock and completes the batches in flight, like the other views.
 *                  Single-node contexts (HDRF_E_UNSUPPORTED when n_ranks > 1).  It needs no recipes:
 *                  live means "a live index entry of the current epoch names it", so the intended
 *                  sequence is hdrf_block_delete ... hdrf_gc ... hdrf_compact.
 *   Returns        the number of rows with status 0, or a call-level failure that changes nothing:
 *                  HDRF_E_INVAL (null context, n outside [0, HDRF_COMPACT_MAX], n > 0 without ids or
 *                  rows, a duplicate id, unknown flags), HDRF_E_NOMEM (the staging: container_max
 *                  bytes per container), HDRF_E_CAPACITY (out is given and the files of the status-0
 *                  rows do not fit in out_cap; *need is their total).  rows[i] answers ids[i], and one
 *                  failing row does not stop the others: HDRF_E_NOTFOUND (neither arena-resident nor
 *                  loaded), HDRF_E_INVAL (open, or with retain_containers closed and not yet drained:
 *                  hdrf_drain_containers first), HDRF_E_DEVICE (the live ranges that name it overlap,
 *                  or one is empty or reaches past the container's bytes), 2 (no live entry names it:
 *                  the DataNode deletes the file), 1 (the live ranges already tile the container),
 *                  0 (compacted).  A container whose status is not 0 is left exactly as it was; its row
 *                  has moved_chunks 0, file_bytes 0, data_off -1, and new_bytes = old_bytes (status 1
 *                  or HDRF_E_DEVICE) or 0 (status 2); a row the host maps refuse is all zeros but id,
 *                  status and data_off.
 *   Changes        with HDRF_COMPACT_DRY nothing.  Otherwise, for the status-0 rows: exactly the index
 *                  entries that name the container get their new start / stop, every other field and
 *                  every other entry stays bit-identical (no new epoch, no rebuild).  A loaded
 *                  container's device copy, or an arena-resident container's arena slot (and under
 *                  compressor 2 its Lz4Codec file in the compressed arena), becomes the new image; if
 *                  an id is both, the resident copy is compacted and the loaded one is freed.
 *                  hdrf_stats.closed_raw_bytes / closed_file_bytes go down by the differences for
 *                  arena-resident containers.  The allocator, the open containers, recipes and the
 *                  drain bookkeeping are untouched.  All or nothing: everything is classified, checked,
 *                  gathered and compressed in a staging area first, and only then committed; a failure
 *                  before the commit leaves the context as it was, a HIP failure during it marks the
 *                  context lost (HDRF_E_HIP until hdrf_reset), as hdrf_gc's rebuild does.
 * The file handed out, out[data_off, data_off + file_bytes), is the whole new chunkDir + id file: the
 * raw image, or under compressor 2 the Lz4Codec file of the image exactly as the storer's close writes
 * it.  With out == NULL the compaction still happens and data_off is -1; an arena-resident file can then
 * be read with hdrf_container_read.  The new index values become durable with the caller's next
 * hdrf_index_dump, as after hdrf_gc: the DataNode replaces the files and the dump together. */
#define HDRF_COMPACT_MAX 16    /* containers per call (the staging is container_max bytes each) */
#define HDRF_COMPACT_DRY 1     /* account only: no byte, entry or host record changes */
typedef struct {
    uint32_t id;
    int32_t  status;        /* 0 compacted (DRY: would be); 1 nothing to reclaim; 2 dead: no live entry names it;
                               < 0: HDRF_E_* — not eligible or inconsistent.  Anything but 0: left exactly as it was */
    int64_t  chunks;        /* live index entries that name the container */
    int64_t  moved_chunks;  /* of those, entries whose start changes */
    int64_t  old_bytes;     /* raw length before */
    int64_t  new_bytes;     /* raw length after == sum of stop - start over `chunks` */
    int64_t  file_bytes;    /* new chunkDir file: new_bytes, or the Lz4Codec file's length under compressor 2;
                               DRY under compressor 2: -1 (not computed) */
    int64_t  data_off;      /* the file is out[data_off, data_off + file_bytes); -1 when not handed out */
} hdrf_compact_row;
int64_t hdrf_compact(hdrf_ctx *ctx, int32_t flags, const uint32_t *ids, int32_t n, hdrf_compact_row *rows, uint8_t *out,
                     int64_t out_cap, int64_t *need);

/* The size of the fingerprint table, online.  cfg.index_log2 is only the size the context opens with:
 * hdrf_index_info_get tells how loaded the table is, hdrf_index_resize moves it into a table of another
 * size while the context lives on.  The write path runs at full speed up to about 60 % load (DESIGN.md
 * §7b), so a DataNode watches entries / slots and grows the table by one bit before that line; after
 * deletes, hdrf_gc and hdrf_compact it may shrink the table again.
 * hdrf_index_info_get is a view: it completes the batches in flight and applies a pending
 * hdrf_reset_async, as hdrf_index_count does; `entries` is counted on the device.
 * hdrf_index_resize:
 *   When it runs   it takes the context lock, completes the batches in flight and applies a pending
 *                  hdrf_reset_async, like the other views (a context an earlier failure marked lost
 *                  answers as they do).  Single-node contexts (HDRF_E_UNSUPPORTED when n_ranks > 1).
 *                  An open packet receive is allowed, unlike hdrf_gc and hdrf_reset: a receive buffer
 *                  holds block bytes only, and hdrf_append_packet reads and writes neither the table
 *                  nor its size, so receivers may keep appending while the call runs.
 *   Arguments      new_log2 outside [10, 31]: HDRF_E_INVAL.  new_log2 equal to the current size: 0,
 *                  nothing happens.  HDRF_E_CAPACITY when entries * 4 > 3 * 2^new_log2: a table more
 *                  than 75 % full is one the write path cannot use (that line lies between the 60 % at
 *                  which claim still runs at full speed and the 80 % at which it ran 3.4x slower), so
 *                  a shrink never produces one; growing never trips it.  HDRF_E_NOMEM when the new
 *                  table cannot be allocated: both tables are resident during the call.
 *   Changes        afterwards the table has 2^new_log2 slots and holds exactly the live entries it
 *                  held before, each one's 64 bytes unchanged (tag, batch, nCopy, container, start,
 *                  stop, digest bytes, the batch-local fields as they stood): only the slot an entry
 *                  sits in differs.  No new epoch; the batch counter, allocator, arena, recipes, loaded
 *                  containers, drain bookkeeping, receive buffers and stats are untouched, so a later
 *                  write deduplicates against the moved entries exactly as it would have against the
 *                  old table, and hdrf_index_dump returns the same rows.  hdrf_probe_stats speaks of
 *                  slots of the table the last batch ran in: after a resize it reports zeros
 *                  (chunks = 0) until a batch has completed in the new table.
 *   All or nothing the live entries are counted, the load rule checked, the new table allocated,
 *                  cleared and filled, its live entries counted; only when the two counts agree and
 *                  the fill reported no error does the context switch to the new table and free the
 *                  old one.  Any failure before that (HDRF_E_NOMEM, HDRF_E_HIP, or HDRF_E_DEVICE when
 *                  the counts disagree) frees the new table and leaves the context exactly as it was:
 *                  the old table is only ever read, so there is no lost state.
 * Nothing extra makes the new size durable: hdrf_index_dump does not depend on the capacity. */
typedef struct {
    int32_t index_log2;      /* the table's capacity now: 2^index_log2 slots */
    int32_t reserved;        /* 0 */
    int64_t slots;           /* 1 << index_log2 */
    int64_t entries;         /* live entries (== hdrf_index_count) */
    int64_t table_bytes;     /* slots * 64 */
} hdrf_index_info;
int hdrf_index_info_get(hdrf_ctx *ctx, hdrf_index_info *out);
int hdrf_index_resize(hdrf_ctx *ctx, int32_t new_log2);

/* Device memory helpers for callers without their own allocator (bench, tests). */
int hdrf_dev_alloc(hdrf_ctx *ctx, uint64_t bytes, void **out);
int hdrf_dev_free(hdrf_ctx *ctx, void *p);
int hdrf_memcpy_h2d(hdrf_ctx *ctx, void *dst, const void *src, uint64_t bytes);
int hdrf_memcpy_d2h(hdrf_ctx *ctx, void *dst, const void *src, uint64_t bytes);
int hdrf_synchronize(hdrf_ctx *ctx);

/* Synthetic corpus generator (BASELINE config 2; spec in DESIGN.md §Corpus):
 * block b, segment s = splitmix64 words keyed by roots[b*segs_per_block+s]. */
int hdrf_corpus_fill(hdrf_ctx *ctx, uint8_t *dev, const uint32_t *roots_host, int64_t nblocks,
                     int64_t segs_per_block, int64_t seg_bytes, uint64_t seed);
/* Same with mixed != 0: BASELINE config 4's mixed-entropy segments (random / text / binary). */
int hdrf_corpus_fill_kind(hdrf_ctx *ctx, uint8_t *dev, const uint32_t *roots_host, int64_t nblocks,
                          int64_t segs_per_block, int64_t seg_bytes, uint64_t seed, int32_t mixed);

/* Per-stage device time (ms) accumulated since the last reset, measured with HIP events on
 * the streams the stages run on (cfg.timing = 1): [0] lane_walk_kernel, [1] stitch (repair / path /
 * count / scan / copy / fallback), [2] sha_full_kernel, [3] sha_tail_kernel, [4] idx_claim_kernel,
 * [5] idx_apply_kernel, [6] idx_slow+decide, [7] new-byte scans, [8] flush_kernel, [9] place_kernel,
 * [10] lz4 (compressor 2), [11] gmax2_kernel (granule maxima); node-global contexts also
 * [12] local aggregation + X1 records, [13] owner claim..finish, [14] gx_decide, [15] flush function,
 * [16] device allocator scan, [17] placement (part 1), [18] commit, and the gaps on the back stream
 * that the caller's exchanges fill: [19] X1 (+ the host), [20] X2, [21] descriptor all-gather,
 * [22] X3 (+ the host); [7] / [8] / [9] are the scans, the flush walk and the arena copy. */
int hdrf_stage_times(hdrf_ctx *ctx, double *ms, int32_t n, int32_t reset);
/* Reduction totals since the last reset (this context's blocks): the dedup / compression ratio
 * of the node is logical_bytes / (closed_file_bytes + open_bytes [+ recipe_bytes]). */
typedef struct {
    int64_t blocks, chunks;
    int64_t logical_bytes;       /* bytes of the reduced blocks */
    int64_t new_bytes;           /* sum of storeSize (DataDeduplicator.storeSize :355) */
    int64_t closed_containers;
    int64_t closed_raw_bytes;    /* container bytes of closed containers */
    int64_t closed_file_bytes;   /* their file sizes (Lz4Codec stream under compressor 2) */
    int64_t open_bytes;          /* raw bytes of the open containers (lastBlockID[0..2]) */
    int64_t recipe_bytes;        /* recipes: BE32 size + digests (storeDB :372-392) */
} hdrf_stats;
int hdrf_get_stats(hdrf_ctx *ctx, hdrf_stats *out);

/* Reset the index, containers, allocator and recipes (a fresh DataNode + Redis); completes
 * the batches in flight first.  HDRF_E_INVAL while a packet receive is open (hdrf_rx_begin not
 * yet followed by hdrf_submit_slot or hdrf_rx_cancel). */
int hdrf_reset(hdrf_ctx *ctx);
/* The same without completing the batches in flight: they complete against the old state, and the
 * next submit (node-global contexts: the next hdrf_gx_front_launch, every rank alike) starts the fresh
 * DataNode, so its front half overlaps the old batches' back halves.  Node-global contexts make the
 * switch in that batch's hdrf_gx_owner (the old batches' owner phases, enqueued after this call, still
 * use the old index epoch) and reset the host side in its hdrf_gx_place_wait.  Views and restores (hdrf_index_*, hdrf_*_load, reconstruct, container
 * reads, hdrf_scrub, hdrf_synchronize) complete every batch first, as always, and a reset still pending then (no
 * submit since) is applied before they run, so they see the fresh DataNode and a restore is kept.
 * cfg.retain_containers: drain the old batches' containers as they complete (hdrf_wait_batch,
 * hdrf_drain_containers); while any old container (closed, or bytes of an open one) is not handed
 * out, hdrf_wait_batch on the fresh DataNode's first batch fails with HDRF_E_INVAL and leaves that
 * batch in flight (drain, then wait again), and the views above fail with HDRF_E_INVAL (a view that
 * must complete the batch anyway drops those containers and marks the context for hdrf_reset,
 * HDRF_E_CAPACITY). */
int hdrf_reset_async(hdrf_ctx *ctx);

/* ---- Node-global index over n_ranks GPUs (BASELINE config 3) -------------------
 * All DataNodes of one host share one Redis (JedisPool("localhost"), DN/DataDeduplicator.java:119),
 * one "blockID" allocator (:165-172,:389), one chunkDir and one FIFO (:124-158): the node is ONE
 * reduction over the global block sequence.  With n_ranks > 1 each context owns the index
 * partition {digest : first digest word mod n_ranks == rank} and reduces the blocks it receives;
 * a global batch is rank-major (rank r's blocks take batch positions [gbase_r, gbase_r + nblocks_r)).
 * The caller moves the records between ranks (all-to-all over RCCL/xGMI, hdrf_amd/node.py).
 * Buffers are device pointers laid out [n_ranks][cap][words] (region d = peer d); counts are
 * host int64[n_ranks].  Per global batch, every rank calls, in order:
 *   hdrf_gx_front  -> X1 send (records for each owner)      all-to-all X1
 *   hdrf_gx_owner  <- X1 recv, -> X2 send (responses)        all-to-all X2 (reverse counts)
 *   hdrf_gx_decide <- X2 recv
 *   hdrf_gx_flush_fn -> this rank's flush descriptor             all-gather of the descriptors
 *   hdrf_gx_alloc_scan <- every rank's descriptor: its allocator in + the node's after the batch
 *                     (or the device forms: hdrf_gx_flush_fn_dev / hdrf_gx_alloc_scan_dev)
 *   hdrf_gx_flush  <- alloc_in (from the scan; or, without the scan, rank r gets rank r-1's
 *                     state over a rank-to-rank chain, rank 0 the node's)
 *   hdrf_gx_place  -> X3 send (locations of new entries)     all-to-all X3 (receive counts from
 *                     hdrf_gx_x3_counts: no count exchange)
 *   hdrf_gx_commit <- X3 recv
 * hdrf_reduce_block / hdrf_reduce_batch return HDRF_E_INVAL on such a context. */
#define HDRF_ALLOC_STATE_BYTES 128
typedef struct {
    int64_t cap;             /* records per peer region (all three exchanges) */
    int32_t x1_words;        /* u32 words per X1 record (digest words + batch position + count) */
    int32_t x2_words;        /* 2: owner slot, flags */
    int32_t x3_words;        /* 4: owner slot, container id, start, stop */
    int32_t depth;           /* node-global batches in flight (fronts launched ahead, HDRF_GX_DEPTH) */
    int64_t fn_bytes;        /* bytes of one rank's packed flush descriptor (hdrf_gx_flush_fn_dev) */
} hdrf_gx_layout;
int hdrf_gx_layout_get(hdrf_ctx *ctx, hdrf_gx_layout *out);
int hdrf_gx_front(hdrf_ctx *ctx, int32_t nblocks, const uint8_t *const *dev_data, const uint64_t *len,
                  const uint64_t *readable, const uint64_t *block_ids, uint32_t gbase, uint32_t *x1_send,
                  int64_t *send_counts);
/* hdrf_gx_front split in two: launch the front halves of the next batches (chunking on one stream,
 * SHA on a second, the local aggregation and X1 records on a third, each batch in its own slot)
 * before running the oldest batch's owner .. commit phases (the back stream), then wait for the
 * oldest launched front's X1 send counts.  At most hdrf_gx_layout.depth batches are in the
 * node-global pipeline (launched and not committed); fronts are waited and backs run in launch
 * order.  A slot is reused only after its previous batch's back phases finished on the device. */
int hdrf_gx_front_launch(hdrf_ctx *ctx, int32_t nblocks, const uint8_t *const *dev_data, const uint64_t *len,
                         const uint64_t *readable, const uint64_t *block_ids, uint32_t gbase, uint32_t *x1_send);
int hdrf_gx_front_wait(hdrf_ctx *ctx, int64_t *send_counts);
int hdrf_gx_owner(hdrf_ctx *ctx, const uint32_t *x1_recv, const int64_t *recv_counts, uint32_t *x2_send);
int hdrf_gx_decide(hdrf_ctx *ctx, const uint32_t *x2_recv);
/* The container allocator of a node-global batch without a rank-to-rank chain.  Each storer
 * range's flush walk (DN/DataDeduplicator.java:702-818: close when curPos + len > maxSize) depends
 * on the allocator a rank receives only through the open container's fill; hdrf_gx_flush_fn
 * (after hdrf_gx_decide) tabulates that function on the GPU into desc (int64 words; returns the
 * count, or -(count + 1000) when cap is too small).  With every rank's descriptor (rank order,
 * concatenated, lens[n_ranks]) hdrf_gx_alloc_scan computes this rank's incoming allocator
 * (alloc_in, the exclusive scan from the state after the previous batch) and the node's state
 * after the batch (alloc_final); hdrf_gx_place verifies the prediction against the flush walk. */
int64_t hdrf_gx_flush_fn(hdrf_ctx *ctx, int64_t *desc, int64_t cap);
int hdrf_gx_alloc_scan(hdrf_ctx *ctx, const int64_t *descs, const int64_t *lens, uint8_t *alloc_in,
                       uint8_t *alloc_final);
/* alloc_in: HDRF_ALLOC_STATE_BYTES from the previous rank or the scan (NULL: this context's own
 * state); alloc_out receives the state after this rank's blocks (NULL after a scan: no host
 * round trip). */
int hdrf_gx_flush(hdrf_ctx *ctx, const uint8_t *alloc_in, uint8_t *alloc_out);
/* The allocator scan without host round trips (the back stream's order only): hdrf_gx_flush_fn_dev
 * (after hdrf_gx_decide) writes this rank's flush function as a fixed-size descriptor of
 * hdrf_gx_layout.fn_bytes into dev_desc; the caller all-gathers the G descriptors into dev_descs
 * (rank order, G x fn_bytes, e.g. an RCCL all-gather enqueued on hdrf_gx_stream); then
 * hdrf_gx_alloc_scan_dev composes them on the device from the node's allocator after the previous
 * batch, and hdrf_gx_flush(ctx, NULL, NULL) and hdrf_gx_place(ctx, NULL, ...) use the result
 * (hdrf_gx_place checks the flush walk against the scan's prediction). */
int hdrf_gx_flush_fn_dev(hdrf_ctx *ctx, void *dev_desc);
int hdrf_gx_alloc_scan_dev(hdrf_ctx *ctx, const void *dev_descs);
/* alloc_final: the node's state after the last rank's flush (becomes this context's state; NULL
 * after hdrf_gx_alloc_scan_dev, which computed it).  hdrf_gx_place = hdrf_gx_place_launch (placement,
 * X3 records and their read-back on the back stream, the arena copy on a stream of its own) +
 * hdrf_gx_place_wait (waits for the read-back: this rank's X3 send counts; the scan and the X3
 * counts are checked, the batch's hdrf_batch_* views become valid). */
int hdrf_gx_place(hdrf_ctx *ctx, const uint8_t *alloc_final, uint32_t *x3_send, int64_t *send_counts);
int hdrf_gx_place_launch(hdrf_ctx *ctx, const uint8_t *alloc_final, uint32_t *x3_send);
int hdrf_gx_place_wait(hdrf_ctx *ctx, int64_t *send_counts);
/* Node-global compressor 2 (between hdrf_gx_place and hdrf_gx_commit): every rank's allocator
 * state before and after its flush walk (hdrf_gx_alloc_io, 128 B each; all-gathered by the caller,
 * they tell every rank which rank holds which bytes of each container); the head pieces of a
 * container another rank closes are copied out of / into arena slots (hdrf_gx_piece: write = 0 reads
 * the bytes [off, off + n) of container id into dev and returns when they are there; write = 1
 * enqueues the copy from dev on the back stream and returns at once, so dev must stay valid until
 * hdrf_gx_compress has returned, which runs after the copies); then each rank compresses the
 * containers its flush walk closed (hdrf_gx_compress: the Lz4Codec files of DN/DataDeduplicator.java
 * :748-797, returns how many).  hdrf_amd/node.py plans and runs the transfers. */
int hdrf_gx_alloc_io(hdrf_ctx *ctx, uint8_t *alloc_in, uint8_t *alloc_out);
int hdrf_gx_piece(hdrf_ctx *ctx, uint32_t id, uint64_t off, uint64_t n, void *dev, int32_t write);
int hdrf_gx_compress(hdrf_ctx *ctx);
/* X3 receive counts (int64[n_ranks]) implied by this owner's hdrf_gx_owner decisions: one location
 * per entry created this batch, from the rank holding its minimum block.  Valid from hdrf_gx_place to
 * hdrf_gx_commit; hdrf_gx_commit refuses (HDRF_E_DEVICE) receive counts that differ from them. */
int hdrf_gx_x3_counts(hdrf_ctx *ctx, int64_t *recv_counts);
/* Enqueued on the back stream and not waited for: a device error it raises is reported by the next
 * hdrf_gx_place or by hdrf_gx_sync. */
int hdrf_gx_commit(hdrf_ctx *ctx, const uint32_t *x3_recv, const int64_t *recv_counts);
/* Complete every node-global batch in flight on this rank (all streams); reports a commit error. */
int hdrf_gx_sync(hdrf_ctx *ctx);
/* The stream the back phases (hdrf_gx_owner .. hdrf_gx_commit) run on (a hipStream_t).  A caller
 * that enqueues its X1 / X2 record exchanges on it (RCCL collectives issued on this stream,
 * torch.cuda.ExternalStream in hdrf_amd/node.py) needs no host synchronisation between an exchange
 * and the phase that reads its receive buffer: hdrf_gx_owner and hdrf_gx_decide only enqueue, and
 * a device error they raise is reported by hdrf_gx_place. */
int hdrf_gx_stream(hdrf_ctx *ctx, void **stream);

#ifdef __cplusplus
}
#endif
#endif
