// ctx.hpp — the context behind the C-ABI (include/hdrf.h) and the host functions its translation
// units share.  Internal: included only by the api*.hip files (api.hip core and batch pipeline,
// api_rx.hip packet receive, api_stream.hip stream codecs, api_gx.hip node-global phases,
// api_views.hip views / restore / drain / reconstruction, api_seek.hip seek tables,
// api_verify.hip scrub, api_gc.hip block deletion and index garbage collection, api_compact.hip
// container compaction, api_resize.hip online table resize); each of them names in its header
// comment the context state it may write.  Everything here but hdrf_ctx itself lives in
// hdrf::host, hidden from the library's dynamic symbols.
#pragma once
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <set>
#include <string>
#include <vector>

#include "../../include/hdrf.h"
#include "launchers.hpp"

namespace hdrf {
namespace host __attribute__((visibility("hidden"))) {

constexpr int kStages = hdrf::kNumStages;
constexpr uint64_t kSlack = 64;  // readable bytes required past each block end
constexpr int kSlots = 5;         // batches in flight (walk | SHA | index+store | LZ4 passes)
constexpr int kErrCapacity = 2 | 4 | 8 | 16 | 32;  // device error bits that mean "a buffer is too small"

struct ContainerInfo {
    uint32_t slot;
    uint32_t len;
    int closed;
    uint32_t clen;           // compressor 2, closed: Lz4Codec file length (compressed arena slot)
};

// Per-batch buffers (device) and read-back (pinned host) of one pipeline slot.
struct Slot {
    BlockDesc *d_blocks = nullptr;
    uint32_t *d_spec = nullptr;
    SegMeta *d_meta = nullptr;
    uint8_t *d_gm = nullptr;                  // granule maxima [B][gstride] (chunking pass 1)
    int gstride = 0;
    int64_t max_len = 0;                      // longest block of the batch in this slot
    int max_nseg = 0;                         // most segments of one block of the batch
    uint32_t *d_irr = nullptr;                // irregular-boundary bitmask (meta_cap / 32 + 2 words)
    PathInfo *d_path = nullptr;               // [B]
    int *d_jx = nullptr;                      // [B][jcap]
    uint32_t *d_jt = nullptr;                 // [B][jcap]
    int jcap = 0;
    uint32_t *d_wgsum = nullptr;              // [B][maxw_cap]
    int maxw_cap = 0;
    int *d_rq = nullptr, *d_rq_count = nullptr;   // failed speculative boundaries (repair queue), meta_cap entries
    uint32_t *d_rqkeep = nullptr;             // [kRqKeep][64] cuts of the short repair walks
    size_t spec_words = 0, meta_cap = 0;      // capacity of d_spec (u32) / d_meta (segments), grown on demand
    int total_waves = 0, total_segs = 0, spec_cap = 0;   // lane walk of the batch in this slot
    BlockState *d_bst = nullptr;
    uint32_t *d_off = nullptr, *d_dig = nullptr, *d_slot = nullptr, *d_pre = nullptr;
    uint8_t *d_flags = nullptr;
    uint8_t *d_dcnt = nullptr;                // designated chunks: blocks of the batch holding the digest
    uint32_t *d_tilesum = nullptr, *d_tilepre = nullptr;
    uint64_t *d_store = nullptr;
    RangeState *d_rstate = nullptr;
    FlushEv *d_ev = nullptr;
    ClosedRec *d_closed = nullptr;
    uint32_t *d_nclosed = nullptr;
    uint32_t *d_coll = nullptr, *d_ncoll = nullptr;
    uint32_t *d_pcid = nullptr, *d_ppos = nullptr, *d_queue = nullptr;
    uint32_t *d_segclen = nullptr, *d_filelen = nullptr;
    uint32_t *d_lzwork = nullptr;             // compressor 2: the LZ4 pass's two item counters
    int *d_err = nullptr;
    // pinned read-back, filled by stream B before back_done
    BlockState *h_bst = nullptr;
    uint64_t *h_store = nullptr;
    AllocState *h_alloc = nullptr;
    int *h_err = nullptr;
    uint32_t *h_nclosed = nullptr;
    uint32_t *h_long = nullptr;               // the batch held chunks for the long SHA lanes (queue[64])
    ClosedRec *h_closed = nullptr;
    uint32_t *h_filelen = nullptr;
    BlockDesc *h_desc = nullptr;
    // host metadata of the batch in this slot
    std::vector<uint64_t> ids, lens;
    int nblocks = 0;
    bool pending = false;
    uint32_t close_bound = 0;                 // durable containers: closes this batch may make per range
    uint32_t lz_bound = 0;                    // compressor 2: closes this batch may make per range (LZ4 lag)
    hipEvent_t placed = nullptr;              // compressor 2: the batch's place kernel finished (stream B2)
    hipEvent_t idx_done = nullptr;            // index stage (claim .. finalize) of the batch done (stream B)
    hipEvent_t lz_done = nullptr;             // compressor 2: its closed containers are Lz4Codec files
    uint32_t rx_release = 0;                  // packet path: receive buffers (bit mask) freed when the batch completes
    uint32_t gx_batch = 0;                    // node-global: index batch id of the batch in this slot
    bool gx_compressed = false;               // node-global compressor 2: hdrf_gx_compress ran for the batch
    RecipeCopy *h_rjobs = nullptr, *d_rjobs = nullptr;   // recipe copies of the batch (storeDB)
    hipEvent_t recipe_done = nullptr;         // the copies read d_dig: the slot's next SHA waits
    bool recipe_pending = false;
    bool gen_reset = false;                   // the batch starts a fresh index generation (hdrf_reset_async)
    hipEvent_t walk_done = nullptr, front_done = nullptr, back_done = nullptr, gmax_done = nullptr;
    hipEvent_t copy_done = nullptr;          // host path: the batch's H2D copies landed
    uint8_t *d_hstage = nullptr;              // host path: device copies of the batch's blocks
    uint64_t hstage_stride = 0;
    hipEvent_t evW[4] = {}, evA[3] = {}, evB[10] = {};   // stage markers (timing)
    // node-global mode: the slot's host side of a batch (pinned: front counts, count uploads, the
    // place read-back), whether a batch used the slot, and whether its arena copy ran on stream B2
    struct GxHost *h_gx = nullptr;
    std::vector<int64_t> gx_c1;               // X1 send counts of the batch in the slot
    bool gx_inuse = false, gx_split = false;
    hipEvent_t gx_meta = nullptr;             // placement (part 1) and its read-back done (stream B)
};

// Pinned per-slot exchange with the host in node-global mode: what hdrf_gx_front_wait and
// hdrf_gx_place_wait read, and the receive counts hdrf_gx_owner / hdrf_gx_commit upload (a pageable
// source would make hipMemcpyAsync wait for the stream).
struct GxHost {
    unsigned long long front_cnt[64];         // X1 records emitted per owner (gx_emit)
    int front_err, commit_err;
    int64_t up_r1[64], up_r3[64];             // X1 / X3 receive counts (uploads)
    unsigned long long c3[64], x3e[64], x3want[64];   // X3 send counts, X3 receive counts, X2-implied sends
    AllocState st[4];                         // [0] allocator in [1] predicted [2] node final [3] flush walk result
};

// Per-batch timing of the node-global phases (cfg.timing): HIP events on the streams each phase runs
// on, in a ring indexed by the batch's sequence number, collected once the batch has completed.
enum GxEv {
    kW0 = 0, kA0 = 4, kX0 = 7, kG0 = 11, kG1, kG2, kG3, kG4, kG5, kG6, kG7, kG8, kG9, kG10, kG11, kG12, kG13,
    kP0, kP1, kGxEv
};
constexpr int kGxRing = 8;
struct GxTime {
    hipEvent_t ev[kGxEv] = {};
    uint32_t rec = 0;                         // bit e: ev[e] was recorded for this batch
};

}  // namespace host
}  // namespace hdrf

using namespace hdrf;
using namespace hdrf::host;

struct hdrf_ctx {
    hdrf_cfg cfg{};
    int H = 20, HW = 5;
    hipStream_t st = nullptr;    // stream A: SHA stage (also every synchronous helper)
    hipStream_t stB = nullptr;   // stream B: back stage, index part (and the node-global phases)
    hipStream_t stB2 = nullptr;  // stream B2: back stage, store part (scan, flush, place, read-back)
    hipStream_t stW = nullptr;   // stream W: chunking stage
    hipStream_t stG = nullptr;   // stream G: the granule-max pass (HDRF_GMAX_STREAM), ahead of W
    hipStream_t stC = nullptr;   // stream C: H2D copies of host-submitted batches
    hipStream_t stD = nullptr;   // stream D: container drain D2H (beside the H2D copies on C)
    hipStream_t stR = nullptr;   // stream R: recipe copies once host batches use stream C (there a
                                 // kernel waited for CU slots and stalled the next batch's H2D copies)
    bool host_copies = false;    // hdrf_submit_host / hdrf_rx_begin ran: stream C carries H2D copies
    XferJob *h_xfer = nullptr;   // drain copy jobs (pinned, read by xfer_kernel)
    int xfer_cap = 0;
    hipStream_t stL[2] = {};     // compressor 2: LZ4 streams, alternating by batch (off stream B)
    // chunks >= 64 KiB were seen in the last completed batch: sha_full hashes them on dedicated
    // lanes (sha.hip); off otherwise, where the scan for them costs config 2 ~3 %
    bool sha_long = false;
    int n_cu = 256;                                  // compute units of the device (the scrub hash grid)
    int max_batch = 0, cap_blk = 0, ntiles = 0, ev_cap = 0, closed_cap = 0, coll_cap = 0;
    Slot sl[kSlots];
    uint64_t nsub = 0, nwait = 0;  // batches submitted / completed
    int res = 0;                   // slot of the last completed batch (hdrf_batch_* views)
    // node state (shared by all batches)
    IndexEntry *d_tab = nullptr;
    uint8_t *d_arena = nullptr;
    uint8_t *d_carena = nullptr;                 // compressor 2: Lz4Codec files of closed containers
    uint64_t cslot = 0;
    AllocState *d_alloc = nullptr;
    uint8_t *d_stage = nullptr;
    uint64_t stage_cap = 0;
    uint8_t *d_rd = nullptr;                     // reconstruction scratch (grows)
    uint64_t rd_cap = 0;
    // host state
    uint32_t batch = 0;                              // batch ids: grow over the context's life (never reset)
    uint32_t epoch = 1;                              // index generation in the tag words (1..255)
    uint32_t bfirst = 1;                             // first batch id of the current epoch
    bool gen_pending = false;                        // hdrf_reset_async: the next submit starts a generation
    bool gen_clear = false;                          //   ... whose epoch wrapped (the table is cleared)
    uint32_t scratch_epoch[kSlots] = {};             // node-global: generation of each scratch table
    int have_alloc = 0;
    int last_nblocks = 0;
    bool probe_stale = false;                        // hdrf_index_resize ran since the last completed batch: its
                                                     // slot numbers (Slot::d_slot) are the old table's (hdrf_probe_stats)
    AllocState h_alloc{};
    std::map<uint32_t, ContainerInfo> containers;   // container id -> arena slot
    std::map<uint32_t, uint32_t> slot_owner;         // arena slot -> container id
    // recipes (SET longToBytes(blockId,4) -> BE32 size | digests) live in HBM: digests in an
    // append-only store of 256 MiB chunks, the host keeps only where each one is
    struct RecipeLoc { uint32_t chunk; uint64_t off; uint32_t n; };
    std::vector<uint8_t *> rchunks;
    uint32_t rcur = 0;                                // chunk being filled
    uint64_t rhead = 0;                               // bytes used in it
    std::map<uint32_t, RecipeLoc> recipes;
    std::map<uint32_t, int64_t> lengths;              // block length (recipe head)
    // seek tables (hdrf_seek_build, api_seek.hip): end[] of a stored recipe, u32 per chunk, in an
    // append-only device store of its own (the recipe store stays digests end to end: hdrf_gc walks
    // it); the host keeps where each table is.  minlen: the smallest length among chunks 0..n-2.
    struct SeekLoc { uint32_t chunk; uint64_t off; uint32_t n; uint32_t minlen; };
    std::vector<uint8_t *> schunks;
    uint32_t scur = 0;                                // chunk being filled
    uint64_t shead = 0;                               // bytes used in it
    std::map<uint32_t, SeekLoc> seeks;
    int64_t seek_last_rows = 0, seek_last_reqs = 0;   // the last read call (hdrf_seek_info)
    struct Loaded { uint8_t *ptr; uint64_t len; };
    std::map<uint32_t, Loaded> loaded;               // containers loaded back from files (read side)
    // node-global index (gx.hip): scratch aggregation table, owner-side per-record arrays
    int G = 1, rank = 0;
    // Two batches can be in the node-global pipeline: the front half of batch k+1 (slot (k+1)%2,
    // stream A) runs while batch k goes through its exchanges and back phases (slot k%2, stream B).
    IndexEntry *d_scratch[kSlots] = {};         // per-slot local aggregation table
    int scratch_log2 = 0;
    int64_t gx_cap = 0;
    int gx_depth = 3;                            // node-global batches in flight (HDRF_GX_DEPTH, 2..kSlots)
    hipStream_t stX = nullptr;                   // node-global: local aggregation + X1 records (front)
    unsigned long long *d_gxe[kSlots] = {};      // [G] X1 records emitted per peer, per slot
    unsigned long long *d_x3want = nullptr;      // [G] X3 records the X2 responses call for (sender check)
    AllocState *d_gxst = nullptr;                // [4] device allocator scan: in, predicted, node final, walk
    int *d_gx_err = nullptr;                     // errors of hdrf_gx_commit (reported by the next place / sync)
    uint64_t fn_bytes = 0, fn_mcap = 0;          // packed flush descriptor (hdrf_gx_flush_fn_dev)
    int gx_dscan = 0;                            // the back batch's allocator came from the device scan
    bool gx_place_pending = false;               // hdrf_gx_place_launch ran, hdrf_gx_place_wait not yet
    GxTime gxt[kGxRing];
    uint64_t gxt_done = 0;                       // batches whose phase times were collected
    unsigned long long *d_gx_counts = nullptr;   // [G] X3 records emitted per peer (back phases)
    int64_t *d_gx_rcounts = nullptr;             // [G] records received per peer
    // [G] X3 records each source will send this owner: one per record that holds its created entry's
    // minimum block (own_decide), so the X3 receive counts need no exchange of their own
    unsigned long long *d_gx_x3exp = nullptr;
    std::vector<int64_t> gx_x3recv;
    uint32_t *d_oslot = nullptr;
    uint8_t *d_oflags = nullptr;
    const uint32_t *gx_x2 = nullptr;             // responses of the back batch (caller's buffer)
    AllocState gx_ain{}, gx_aout{};              // allocator before / after this rank's flush walk
    AllocState gx_expect{};                      // this rank's flush result predicted by hdrf_gx_alloc_scan
    int gx_scanned = 0;                          // the back batch's allocator came from the scan
    uint8_t *d_fn = nullptr;                     // flush-function scratch (hdrf_gx_flush_fn)
    uint64_t fn_cap = 0;
    uint64_t gx_nfront = 0, gx_nfwait = 0, gx_nback = 0;   // fronts launched / waited, batches committed
    int gx_bphase = 0;                           // back batch: 0 owner next, 1 decide, 2 flush, 3 place, 4 commit
    hdrf_stats stats{};                          // cumulative since the last reset
    uint32_t lzop_mtime = 0;                     // stream codec 3: the lzop header's mtime field
    // concurrency: every entry point holds mu; ticketed reductions also wait for their turn
    // (AIWriteQueue order, DN/DataDeduplicator.java:124-158, DN/DDRunner.java:20-36)
    std::recursive_mutex mu;
    std::condition_variable_any turn;
    uint64_t next_ticket = 0, serving = 0;
    std::set<uint64_t> cancelled;
    // durable containers (cfg.retain_containers): closed containers stay in their arena slot until
    // drained; open containers' bytes already handed out
    std::vector<uint32_t> pend_closed;
    uint32_t undrained[4] = {0, 0, 0, 0};
    uint32_t inflight_bound = 0;
    uint32_t gen_reserve = 0;                 // hdrf_reset_async (durable): the old generation's open slot
    std::map<uint32_t, int64_t> handed;
    bool lost = false;
    // packet-granular receive (hdrf_rx_begin / hdrf_append_packet / hdrf_submit_slot): device
    // receive buffers, and a pinned chunk ring the packets are copied into before their H2D
    static constexpr int kRx = 16;
    // pinned staging chunk per receive buffer (two alternate): 4 MiB, HDRF_RX_CHUNK_MB for A/B
    const uint64_t kRingChunk = [] {
        const char *e = getenv("HDRF_RX_CHUNK_MB");
        const long v = e ? atol(e) : 4;
        return (uint64_t)(v >= 1 && v <= 64 ? v : 4) << 20;
    }();
    // one receive buffer per block being received: device copy of the block, and two pinned 4 MiB
    // staging chunks of its own, so receivers of different blocks (one DataXceiver thread each)
    // copy their packets concurrently, outside the context lock
    struct Rx {
        uint8_t *d = nullptr;                   // device buffer (max_block_bytes + slack)
        uint8_t *h = nullptr;                   // pinned staging, 2 x kRingChunk
        hipEvent_t ev[2] = {nullptr, nullptr};  // H2D of each staging chunk
        bool busy[2] = {false, false};
        hipStream_t st = nullptr;               // HDRF_RX_STREAMS=1: this buffer's own H2D stream
        hipEvent_t done = nullptr;              //   (its copies then never queue behind other receivers')
        int cur = 0;
        uint64_t fill = 0, dst = 0;             // bytes in the current chunk, their block offset
        uint64_t len = 0, id = 0;
        std::atomic<int> state{0};              // 0 free 1 receiving 2 submitted
    };
    Rx rx[kRx];
    bool rx_used = false;                       // a packet receive was opened (drain engine choice)
    // timing
    bool timing = false;
    double stage_ms[kStages] = {};
    std::string err;
};

#define HIPCK(x)                                                                       \
    do {                                                                               \
        hipError_t e_ = (x);                                                           \
        if (e_ != hipSuccess) {                                                        \
            ctx->err = std::string(#x) + ": " + hipGetErrorString(e_);                 \
            return HDRF_E_HIP;                                                         \
        }                                                                              \
    } while (0)

// every entry point: one caller at a time (a null context is checked by the function itself)
#define HDRF_LOCK(c)                                                                                 \
    std::unique_lock<std::recursive_mutex> lk_ =                                                     \
        (c) ? std::unique_lock<std::recursive_mutex>((c)->mu) : std::unique_lock<std::recursive_mutex>()

namespace hdrf {
namespace host __attribute__((visibility("hidden"))) {

// tag key of the index (common.hpp tag_word): the current epoch over the tag-bit mask (all ones
// except under the debug_tag_bits collision hook)
inline unsigned long long tag_bits(const hdrf_ctx *ctx)
{
    const int bits = ctx->cfg.debug_tag_bits;
    return ((bits <= 0 || bits >= 56) ? ~0ull : ((1ull << bits) - 1)) & kTag56;
}
inline unsigned long long tag_mask(const hdrf_ctx *ctx)
{
    return ((unsigned long long)ctx->epoch << 56) | tag_bits(ctx);
}

inline int set_err(hdrf_ctx *ctx, int code, const std::string &msg)
{
    if (ctx) ctx->err = msg;
    return code;
}

template <class T>
inline int dalloc(hdrf_ctx *ctx, T **p, size_t count)
{
    size_t bytes = std::max<size_t>(count * sizeof(T), 256);
    if (hipMalloc((void **)p, bytes) != hipSuccess) {
        *p = nullptr;
        ctx->err = "hipMalloc failed (" + std::to_string(bytes) + " bytes)";
        return HDRF_E_NOMEM;
    }
    return 0;
}

template <class T>
inline int halloc(hdrf_ctx *ctx, T **p, size_t count)
{
    if (hipHostMalloc((void **)p, std::max<size_t>(count * sizeof(T), 64), hipHostMallocDefault) != hipSuccess) {
        *p = nullptr;
        ctx->err = "hipHostMalloc failed";
        return HDRF_E_NOMEM;
    }
    std::memset(*p, 0, std::max<size_t>(count * sizeof(T), 64));
    return 0;
}

inline float elapsed(hipEvent_t a, hipEvent_t b)
{
    float ms = 0;
    return hipEventElapsedTime(&ms, a, b) == hipSuccess ? ms : 0.f;
}

// Stage times of a maintenance call for its speed script (scripts/gc_speed.py, scripts/compact_speed.py):
// when the environment variable `env` is set and not 0 (read at every call; changes no result), mark(i)
// records event i of n on the stream and the call prints the deltas to stderr.
struct StageTimer {
    bool on;
    std::vector<hipEvent_t> ev;
    StageTimer(const char *env, int n) : on(env_int(env, 0) != 0), ev((size_t)n, nullptr)
    {
        for (auto &e : ev)
            if (on && hipEventCreate(&e) != hipSuccess) on = false;
    }
    ~StageTimer()
    {
        for (auto &e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    void mark(int i, hipStream_t st)
    {
        if (on) (void)hipEventRecord(ev[i], st);
    }
    float ms(int a, int b) const { return elapsed(ev[a], ev[b]); }
};

// ---- functions that cross files (callers hold the context lock) ----------------------------
// api.hip
// complete every batch in flight (views, reset, the node-global phases need a quiet context)
int drain(hdrf_ctx *ctx);
// a batch's device error flags as HDRF_E_CAPACITY / HDRF_E_DEVICE, with the message
int device_error(hdrf_ctx *ctx, int herr);
// the allocator of a fresh DataNode
AllocState initial_alloc(const hdrf_ctx *ctx);
// the host side of a fresh DataNode: containers, recipes, allocator view, totals
void reset_host(hdrf_ctx *ctx);
// container id -> slot bookkeeping after a batch
void note_container(hdrf_ctx *ctx, uint32_t id, uint32_t slot, uint32_t len, int closed, uint32_t clen = 0);
// the slot's chunking scratch as the launcher takes it
ChunkScratch chunk_scratch(Slot &S, int compressor = 1);
// validate a batch, fill the slot's descriptors (lane segmentation), grow its speculative lists
int prepare_blocks(hdrf_ctx *ctx, Slot &S, int32_t nblocks, const uint8_t *const *dev_data, const uint64_t *len,
                   const uint64_t *readable);
StoreParams store_params(const hdrf_ctx *ctx, int nblocks);
// the front of a batch (single-GPU and node-global alike): descriptors up on G, chunking on W,
// fingerprints on A
int enqueue_front(hdrf_ctx *ctx, Slot &S, int nblocks, hipStream_t W, hipStream_t G, hipStream_t A, Marker *mw, Marker *ma,
                  bool after_copy = false);
// enqueue one batch: front on stream A, back on stream B
int submit(hdrf_ctx *ctx, int32_t nblocks, const uint8_t *const *dev_data, const uint64_t *len,
           const uint64_t *readable, const uint64_t *block_ids, bool after_copy = false);
// space for one recipe's digests in the device recipe store
int recipe_alloc(hdrf_ctx *ctx, uint64_t bytes, uint32_t key, uint32_t n, uint8_t **dst);
// [BE32 size | digests] out of the device store (the caller drained): 1 found, 0 absent, < 0 error
int fetch_recipe(hdrf_ctx *ctx, uint32_t key, std::vector<uint8_t> &r);
// after a batch's read-back landed: container / recipe / allocator bookkeeping
int complete_slot(hdrf_ctx *ctx, int si, bool timed);
// api_stream.hip
// Hadoop codec file -> the compressed blocks it holds; false if malformed
bool plan_lz4_frame(const uint8_t *f, int64_t n, std::vector<LzDec> &items, uint64_t *raw_total, int codec = 4);
// decode a host-resident Lz4Codec / SnappyCodec file into device memory; returns the raw length
int64_t decode_file(hdrf_ctx *ctx, const uint8_t *file, int64_t flen, uint8_t *dev_out, int64_t cap, int codec = 4);
// api_views.hip
// a device scratch buffer of at least `need` bytes (contents are not kept when it grows)
int grow(hdrf_ctx *ctx, uint8_t **p, uint64_t *cap, uint64_t need);
// The readable containers sorted by id (arena residents, and those loaded back from files where no
// resident has the id), each with the two bounds a reader must respect: `valid`, the bytes the
// container holds (ContainerInfo.len / the loaded file's raw length), and `alloc`, the bytes
// readable from `base` (container_max / raw + 64).
struct Readable {
    std::vector<uint32_t> cid, valid;
    std::vector<uint64_t> base, alloc;
};
void readable_list(const hdrf_ctx *ctx, Readable &r);
// The two test hooks of the scrub / verified reads (verify.hip, api_verify.hip), both read at every
// call so a test can set them between calls; neither changes a result:
//   HDRF_VF_WGS            workgroups (4 waves each) of the persistent hash kernel.  Default: 8 waves
//                          per CU, as the SHA stage runs (4, 6 and 8 measured alike, 12 and 16 slower,
//                          profiles/scrub_speed_20261020.txt).  A wave reserves 64 items at a time, so
//                          only a small grid makes the waves of a small store reserve twice:
//                          tests/test_scrub.py runs with 1.
//   HDRF_SCRUB_SLICE_LOG2  log2 of the table slots per scrub slice (10..22, default 22), so a small
//                          table is walked in several slices.
inline int vf_workgroups(const hdrf_ctx *ctx)
{
    const int w = env_int("HDRF_VF_WGS", 0);
    return w >= 1 ? w : std::max(1, ctx->n_cu * 2);
}
constexpr int kScrubSliceLog2 = 22;
inline int scrub_slice_log2(const hdrf_ctx *ctx)
{
    return std::min(ctx->cfg.index_log2, std::min(kScrubSliceLog2, std::max(10, env_int("HDRF_SCRUB_SLICE_LOG2", kScrubSliceLog2))));
}

}  // namespace host
}  // namespace hdrf
