// api.hip — libhdrf C-ABI (include/hdrf.h): context, batch pipeline, host views.
//
// One context = one DataNode's reduction state on one GPU: the index table (Redis in the
// reference), the container arena (chunkDir files), the allocator ("blockID" key) and the
// recipes.
//
// Batches run as a two-stage pipeline over two HIP streams and two buffer slots:
//   front (stream A): descriptor upload, chunking, SHA            -> per-slot arrays only
//   back  (stream B): index, placement/gather, compression, read-back of the batch's small state
// Batch k's front waits only for the back of batch k-2 (its slot's previous user); its back waits
// for its own front and, by stream order, for batch k-1's back (the index, allocator and arena
// are updated strictly in block order: the reference's FIFO, DN/DataDeduplicator.java:124-158).
// So while batch k is being indexed and stored, batch k+1 is already being chunked and hashed.
// hdrf_submit_batch enqueues; hdrf_wait_batch completes the oldest batch (host bookkeeping);
// hdrf_reduce_batch does both.
//
// This file is the core: it owns the context's life (open / close, every allocation, reset and the
// generation switch), the pipeline counters (nsub, nwait, res, batch, epoch) and the completion
// bookkeeping (containers, recipes, allocator view, stats), and may write any context state.  The
// other subsystems (api_rx.hip, api_stream.hip, api_gx.hip, api_views.hip) reach it through the
// functions ctx.hpp declares.
#include <new>

#include "ctx.hpp"

int host::device_error(hdrf_ctx *ctx, int herr)
{
    std::string m = "device reported error flags " + std::to_string(herr);
    if (herr & 32) m += " (arena_slots too small: a storer range closed more containers in one batch than its ring holds)";
    if (herr & 2) m += " (index table full)";
    if (herr & 1) m += " (chunking: offsets capacity or an unterminated fallback walk)";
    if (herr & 192) m += " (chunking: speculative list overflow / inconsistent stitch)";
    if (herr & 4) m += " (tag-collision list full)";
    if (herr & 256) m += " (node-global: an X3 location names no index entry)";
    if (herr & 512) m += " (node-global: malformed flush descriptor in the allocator scan)";
    if (herr & 1024) m += " (node-global: flush function candidate table overflow or runaway chain)";
    return set_err(ctx, (herr & kErrCapacity) ? HDRF_E_CAPACITY : HDRF_E_DEVICE, m);
}

extern "C" int hdrf_default_cfg(hdrf_cfg *cfg)
{
    if (!cfg) return HDRF_E_INVAL;
    std::memset(cfg, 0, sizeof *cfg);
    cfg->hasher = 0;
    cfg->compressor = 1;
    cfg->window = 700;
    cfg->max_chunk = 1000000;
    cfg->n_thread = 3;
    cfg->min_mt_chunks = 25;
    cfg->container_max = 1u << 25;
    cfg->device = 0;
    cfg->max_block_bytes = 128ll << 20;
    cfg->max_batch_blocks = 8;
    cfg->retain_containers = 0;
    cfg->index_log2 = 22;
    cfg->arena_slots = 16;
    cfg->segment_bytes = 1 << 20;
    cfg->keep_recipes = 1;
    cfg->timing = 0;
    cfg->n_ranks = 1;
    cfg->rank = 0;
    return 0;
}

static void free_slot(Slot &S)
{
    void *dev[] = {S.d_blocks, S.d_spec, S.d_meta, S.d_gm, S.d_irr, S.d_path, S.d_jx, S.d_jt, S.d_wgsum, S.d_rq, S.d_rq_count, S.d_rqkeep, S.d_bst, S.d_off, S.d_dig, S.d_slot,
                   S.d_pre, S.d_flags, S.d_dcnt, S.d_tilesum, S.d_tilepre, S.d_store, S.d_rstate, S.d_ev, S.d_closed,
                   S.d_nclosed, S.d_coll, S.d_ncoll, S.d_pcid, S.d_ppos, S.d_queue, S.d_segclen, S.d_filelen, S.d_err,
                   S.d_lzwork};
    for (void *p : dev)
        if (p) (void)hipFree(p);
    void *host[] = {S.h_bst, S.h_store, S.h_alloc, S.h_err, S.h_nclosed, S.h_long, S.h_closed, S.h_filelen, S.h_desc,
                    S.h_gx};
    for (void *p : host)
        if (p) (void)hipHostFree(p);
    hipEvent_t evs[] = {S.walk_done, S.front_done, S.back_done, S.copy_done, S.recipe_done, S.placed, S.lz_done,
                        S.gmax_done, S.idx_done, S.gx_meta};
    if (S.d_rjobs) (void)hipFree(S.d_rjobs);
    if (S.h_rjobs) (void)hipHostFree(S.h_rjobs);
    if (S.d_hstage) (void)hipFree(S.d_hstage);
    for (auto e : evs)
        if (e) (void)hipEventDestroy(e);
    for (auto e : S.evW)
        if (e) (void)hipEventDestroy(e);
    for (auto e : S.evA)
        if (e) (void)hipEventDestroy(e);
    for (auto e : S.evB)
        if (e) (void)hipEventDestroy(e);
}

static void free_all(hdrf_ctx *ctx)
{
    for (auto &S : ctx->sl) free_slot(S);
    for (auto &kv : ctx->loaded) (void)hipFree(kv.second.ptr);
    ctx->loaded.clear();
    for (auto p : ctx->rchunks) (void)hipFree(p);
    ctx->rchunks.clear();
    for (auto p : ctx->schunks) (void)hipFree(p);
    ctx->schunks.clear();
    void *ptrs[] = {ctx->d_tab, ctx->d_arena, ctx->d_alloc, ctx->d_stage, ctx->d_rd, ctx->d_gx_counts,
                    ctx->d_gx_rcounts, ctx->d_oslot, ctx->d_oflags, ctx->d_carena, ctx->d_fn, ctx->d_gx_x3exp,
                    ctx->d_x3want, ctx->d_gxst, ctx->d_gx_err};
    for (void *p : ptrs)
        if (p) (void)hipFree(p);
    for (int i = 0; i < kSlots; i++) {
        if (ctx->d_scratch[i]) (void)hipFree(ctx->d_scratch[i]);
        if (ctx->d_gxe[i]) (void)hipFree(ctx->d_gxe[i]);
    }
    for (auto &T : ctx->gxt)
        for (auto e : T.ev)
            if (e) (void)hipEventDestroy(e);
    if (ctx->stX) (void)hipStreamDestroy(ctx->stX);
    if (ctx->st) (void)hipStreamDestroy(ctx->st);
    if (ctx->stB) (void)hipStreamDestroy(ctx->stB);
    if (ctx->stB2) (void)hipStreamDestroy(ctx->stB2);
    if (ctx->stW) (void)hipStreamDestroy(ctx->stW);
    if (ctx->stG) (void)hipStreamDestroy(ctx->stG);
    if (ctx->stC) (void)hipStreamDestroy(ctx->stC);
    if (ctx->stD) (void)hipStreamDestroy(ctx->stD);
    if (ctx->stR) (void)hipStreamDestroy(ctx->stR);
    if (ctx->h_xfer) (void)hipHostFree(ctx->h_xfer);
    for (auto L : ctx->stL)
        if (L) (void)hipStreamDestroy(L);
    for (auto &r : ctx->rx)
        if (r.d) (void)hipFree(r.d);
    for (auto &r : ctx->rx) {
        if (r.h) (void)hipHostFree(r.h);
        for (auto e : r.ev)
            if (e) (void)hipEventDestroy(e);
        if (r.done) (void)hipEventDestroy(r.done);
        if (r.st) (void)hipStreamDestroy(r.st);
    }
}

static int alloc_slot(hdrf_ctx *ctx, Slot &S)
{
    const hdrf_cfg &c = ctx->cfg;
    const int B = ctx->max_batch;
    const size_t nchunk = (size_t)B * ctx->cap_blk;
    const int nseg_lz = (int)((c.container_max + 261099) / 261100);
    int rc = 0;
    // speculative lists: sized for one wave of lane segments per 1 MiB of the largest batch, grown
    // on demand when a batch cuts finer (prepare_blocks)
    const int seg_len0 = std::max(kSegMinWin, std::min(kSegMaxWin, (int)(c.segment_bytes / kWaveSegs / (c.window + 2)))) *
                         (c.window + 2);
    S.meta_cap = (size_t)B * (size_t)(c.max_block_bytes / seg_len0 + 2);
    S.spec_words = S.meta_cap * (size_t)lane_spec_cap(seg_len0, c.window);
    S.gstride = (int)(((c.max_block_bytes + 15) / 16 + 1024 + 255) & ~(int64_t)255);
    // on-path stitch jumps: at most one per segment boundary at the finest segmentation
    S.jcap = (int)(c.max_block_bytes / ((int64_t)kSegMinWin * (c.window + 2)) + 2);
    if ((rc = dalloc(ctx, &S.d_blocks, B)) || (rc = dalloc(ctx, &S.d_spec, S.spec_words)) ||
        (rc = dalloc(ctx, &S.d_gm, (size_t)B * S.gstride)) || (rc = dalloc(ctx, &S.d_path, B)) ||
        (rc = dalloc(ctx, &S.d_jx, (size_t)B * S.jcap)) || (rc = dalloc(ctx, &S.d_jt, (size_t)B * S.jcap)) ||
        (rc = dalloc(ctx, &S.d_irr, S.meta_cap / 32 + 2)) ||
        (rc = dalloc(ctx, &S.d_meta, S.meta_cap)) || (rc = dalloc(ctx, &S.d_rq, S.meta_cap)) ||
        (rc = dalloc(ctx, &S.d_rq_count, 1)) || (rc = dalloc(ctx, &S.d_rqkeep, (size_t)kRqKeep * 64)) ||
        (rc = dalloc(ctx, &S.d_bst, B)) ||
        (rc = dalloc(ctx, &S.d_off, nchunk)) || (rc = dalloc(ctx, &S.d_dig, nchunk * ctx->HW)) ||
        (rc = dalloc(ctx, &S.d_slot, nchunk)) ||
        (rc = dalloc(ctx, &S.d_pre, nchunk)) || (rc = dalloc(ctx, &S.d_flags, nchunk)) || (rc = dalloc(ctx, &S.d_dcnt, nchunk)) ||
        (rc = dalloc(ctx, &S.d_tilesum, (size_t)B * ctx->ntiles)) ||
        (rc = dalloc(ctx, &S.d_tilepre, (size_t)B * ctx->ntiles)) || (rc = dalloc(ctx, &S.d_store, B)) ||
        (rc = dalloc(ctx, &S.d_rstate, (size_t)B * 4)) || (rc = dalloc(ctx, &S.d_ev, (size_t)3 * ctx->ev_cap)) ||
        (rc = dalloc(ctx, &S.d_closed, ctx->closed_cap)) || (rc = dalloc(ctx, &S.d_nclosed, 1)) ||
        (rc = dalloc(ctx, &S.d_coll, ctx->coll_cap)) || (rc = dalloc(ctx, &S.d_ncoll, 1)) ||
        (rc = dalloc(ctx, &S.d_pcid, nchunk)) || (rc = dalloc(ctx, &S.d_ppos, nchunk)) ||
        (rc = dalloc(ctx, &S.d_queue, 128)) || (rc = dalloc(ctx, &S.d_err, 1)) ||
        (rc = halloc(ctx, &S.h_bst, B)) || (rc = halloc(ctx, &S.h_store, B)) || (rc = halloc(ctx, &S.h_alloc, 1)) ||
        (rc = halloc(ctx, &S.h_err, 1)) || (rc = halloc(ctx, &S.h_nclosed, 1)) || (rc = halloc(ctx, &S.h_long, 1)) ||
        (rc = halloc(ctx, &S.h_closed, ctx->closed_cap)) || (rc = halloc(ctx, &S.h_filelen, ctx->closed_cap)) ||
        (rc = halloc(ctx, &S.h_desc, B)))
        return rc;
    if (c.compressor == 2 && ((rc = dalloc(ctx, &S.d_segclen, (size_t)ctx->closed_cap * nseg_lz)) ||
                              (rc = dalloc(ctx, &S.d_filelen, (size_t)ctx->closed_cap)) ||
                              (rc = dalloc(ctx, &S.d_lzwork, 2))))
        return rc;
    if ((rc = dalloc(ctx, &S.d_rjobs, B)) || (rc = halloc(ctx, &S.h_rjobs, B))) return rc;
    if (hipEventCreateWithFlags(&S.walk_done, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&S.copy_done, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&S.recipe_done, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&S.front_done, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&S.back_done, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&S.placed, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&S.lz_done, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&S.gmax_done, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&S.idx_done, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&S.gx_meta, hipEventDisableTiming) != hipSuccess)
        return set_err(ctx, HDRF_E_HIP, "hipEventCreate failed");
    for (auto &e : S.evW)
        if (hipEventCreate(&e) != hipSuccess) return set_err(ctx, HDRF_E_HIP, "hipEventCreate failed");
    for (auto &e : S.evA)
        if (hipEventCreate(&e) != hipSuccess) return set_err(ctx, HDRF_E_HIP, "hipEventCreate failed");
    for (auto &e : S.evB)
        if (hipEventCreate(&e) != hipSuccess) return set_err(ctx, HDRF_E_HIP, "hipEventCreate failed");
    if (hipMemsetAsync(S.d_err, 0, sizeof(int), ctx->st) != hipSuccess) return set_err(ctx, HDRF_E_HIP, "memset");
    return 0;
}

static int wait_one(hdrf_ctx *ctx, bool force = false);
static int init_state(hdrf_ctx *ctx, bool fresh);
static bool gen_undrained(const hdrf_ctx *ctx);

// complete every batch in flight (views, reset, the node-global phases need a quiet context)
int host::drain(hdrf_ctx *ctx)
{
    int rc = 0;
    // (forced: a generation switch whose old containers were not drained still completes, and the
    // context is marked lost until hdrf_reset)
    while (ctx->nwait < ctx->nsub)
        if (int r = wait_one(ctx, true)) rc = rc ? rc : r;
    HIPCK(hipStreamSynchronize(ctx->stC));
    if (ctx->stR) HIPCK(hipStreamSynchronize(ctx->stR));
    for (auto L : ctx->stL) HIPCK(hipStreamSynchronize(L));
    HIPCK(hipStreamSynchronize(ctx->stG));
    HIPCK(hipStreamSynchronize(ctx->stW));
    HIPCK(hipStreamSynchronize(ctx->st));
    HIPCK(hipStreamSynchronize(ctx->stB));
    HIPCK(hipStreamSynchronize(ctx->stB2));
    if (ctx->stX) HIPCK(hipStreamSynchronize(ctx->stX));
    if (rc) return rc;
    if (ctx->gen_pending && ctx->gx_nfront == ctx->gx_nback) {
        // hdrf_reset_async with no batch submitted since: the caller of a view or a restore sees the
        // fresh generation it asked for, applied now (a restore is then not undone by the next submit)
        if (ctx->cfg.retain_containers && gen_undrained(ctx))
            return set_err(ctx, HDRF_E_INVAL, "hdrf_reset_async is pending and the previous generation's containers "
                                              "were not drained (hdrf_drain_containers first, or hdrf_reset)");
        return init_state(ctx, false);
    }
    return 0;
}

AllocState host::initial_alloc(const hdrf_ctx *ctx)
{
    AllocState a{};
    for (int t = 0; t < 4; t++) {
        a.id[t] = (uint32_t)t << 22;                 // utilities.bytesToBlockID, absent key (DN/utilities.java:36-50)
        // (node-global mode: the one allocator of the node, carried rank to rank by hdrf_gx_flush)
        a.slot[t] = (uint32_t)t * (uint32_t)(ctx->cfg.arena_slots / 4);   // per-range slot rings
    }
    return a;
}

// the host side of a fresh DataNode: containers, recipes, allocator view, totals
void host::reset_host(hdrf_ctx *ctx)
{
    ctx->h_alloc = initial_alloc(ctx);
    ctx->have_alloc = 0;
    ctx->containers.clear();
    ctx->slot_owner.clear();
    for (auto &kv : ctx->loaded) (void)hipFree(kv.second.ptr);
    ctx->loaded.clear();
    ctx->recipes.clear();
    ctx->rcur = 0;
    ctx->rhead = 0;
    ctx->seeks.clear();                              // (the seek store's chunks are refilled from the start, as the recipes')
    ctx->scur = 0;
    ctx->shead = 0;
    ctx->lengths.clear();
    ctx->stats = hdrf_stats{};
}

static int init_state(hdrf_ctx *ctx, bool fresh)
{
    ctx->gen_pending = false;                        // (before drain: this is the generation switch)
    (void)drain(ctx);
    const AllocState a = initial_alloc(ctx);
    for (auto &S : ctx->sl) HIPCK(hipMemsetAsync(S.d_err, 0, sizeof(int), ctx->st));
    HIPCK(hipStreamSynchronize(ctx->st));
    // the index and allocator belong to the back stream (also for the node-global back phases).
    // A fresh index is a new epoch: every entry tagged with another one is empty (common.hpp), so
    // the 2^k x 64 B table is cleared only at open and once every 255 resets; batch ids keep
    // growing, and the claim rule tells this epoch's entries by batch >= bfirst (index.hip).
    // (gen_clear: a pending hdrf_reset_async already wrapped the epoch)
    hipStream_t ist = ctx->stB;
    const bool clear = fresh || ctx->epoch >= 255 || ctx->gen_clear;
    ctx->gen_clear = false;
    ctx->epoch = clear ? 1 : ctx->epoch + 1;
    if (fresh) ctx->batch = 0;
    ctx->bfirst = ctx->batch + 1;
    HIPCK(launch_index_clear(ctx->d_tab, clear ? ctx->cfg.index_log2 : -1, ctx->d_alloc, a, ist));
    if (fresh)
        for (int i = 0; i < kSlots; i++)
            if (ctx->d_scratch[i]) {
                HIPCK(hipMemsetAsync(ctx->d_scratch[i], 0, sizeof(IndexEntry) << ctx->scratch_log2, ist));
                ctx->scratch_epoch[i] = 0;
            }
    reset_host(ctx);
    for (auto &S : ctx->sl) S.recipe_pending = S.gen_reset = false;
    ctx->last_nblocks = 0;
    ctx->probe_stale = false;
    ctx->gx_nfront = ctx->gx_nfwait = ctx->gx_nback = 0;
    ctx->gx_bphase = 0;
    ctx->gx_dscan = ctx->gx_scanned = 0;
    ctx->gx_place_pending = false;
    ctx->gxt_done = 0;
    for (auto &T : ctx->gxt) T.rec = 0;
    for (auto &S : ctx->sl) S.gx_inuse = S.gx_split = false;
    if (ctx->d_gx_err) HIPCK(hipMemsetAsync(ctx->d_gx_err, 0, sizeof(int), ist));
    ctx->pend_closed.clear();
    for (auto &u : ctx->undrained) u = 0;
    ctx->inflight_bound = 0;
    ctx->gen_reserve = 0;
    ctx->handed.clear();
    ctx->lost = false;
    for (auto &r : ctx->rx) { r.state = 0; r.len = 0; r.fill = 0; r.busy[0] = r.busy[1] = false; }
    for (auto &S : ctx->sl) S.rx_release = 0;
    return 0;
}

extern "C" int hdrf_open(const hdrf_cfg *cfg_in, hdrf_ctx **out)
{
    if (!cfg_in || !out) return HDRF_E_INVAL;
    *out = nullptr;
    const hdrf_cfg &c = *cfg_in;
    if ((c.hasher != 0 && c.hasher != 1) || c.window < 32 || c.window > 1000 || c.max_chunk <= c.window ||
        c.n_thread < 1 || c.n_thread > 3 || c.max_batch_blocks < 1 || c.max_batch_blocks > kMaxBatch ||
        c.index_log2 < 10 || c.index_log2 > 31 || c.arena_slots < 8 || c.max_block_bytes < 1 ||
        c.max_block_bytes > (1ll << 30) || c.container_max <= (uint32_t)c.max_chunk + 1 || c.segment_bytes < (1 << 16) ||
        c.debug_tag_bits < 0 || c.debug_tag_bits > 64 || (c.debug_tag_bits && c.hasher != 0) ||
        c.n_ranks < 1 || c.n_ranks > 64 || c.rank < 0 || c.rank >= c.n_ranks)
        return HDRF_E_INVAL;
    // 1 = dedup, 2 = dedup + Lz4Codec containers (single-node contexts; the node-global mode
    // assembles containers from several GPUs and compresses them in a later step: unsupported yet)
    if (c.compressor != 1 && c.compressor != 2) return HDRF_E_UNSUPPORTED;
    hdrf_ctx *ctx = new (std::nothrow) hdrf_ctx();
    if (!ctx) return HDRF_E_NOMEM;
    ctx->cfg = c;
    ctx->H = c.hasher == 0 ? 20 : 28;
    ctx->HW = c.hasher == 0 ? 5 : 7;
    int rc = 0;
    // Stages per batch: chunking (W, scalar-unit bound), SHA (A, VALU-bound), index + store (B,
    // memory-bound).  By default W is A (two stages: front = chunking + SHA, back = index + store);
    // the front is the critical path, B has slack.  HDRF_PRIO: 1 = W, A high (default), 0 = equal,
    // 2 = B high.
    int lo_prio = 0, hi_prio = 0;
    (void)hipDeviceGetStreamPriorityRange(&lo_prio, &hi_prio);
    const char *pe = std::getenv("HDRF_PRIO");
    const int prio_mode = pe ? std::atoi(pe) : 1;
    // 3 = only A (SHA) high: chunking of a later batch then fills the slots SHA leaves
    const int pa = (prio_mode == 1 || prio_mode == 3) ? hi_prio : lo_prio, pb = prio_mode == 2 ? hi_prio : lo_prio;
    const int pw = prio_mode == 1 ? hi_prio : lo_prio;
    if (hipSetDevice(c.device) != hipSuccess ||
        hipStreamCreateWithPriority(&ctx->st, hipStreamNonBlocking, pa) != hipSuccess ||
        hipStreamCreateWithPriority(&ctx->stB, hipStreamNonBlocking, pb) != hipSuccess ||
        hipStreamCreateWithPriority(&ctx->stB2, hipStreamNonBlocking, pb) != hipSuccess ||
        hipStreamCreateWithPriority(&ctx->stW, hipStreamNonBlocking, pw) != hipSuccess ||
        hipStreamCreateWithPriority(&ctx->stG, hipStreamNonBlocking, pw) != hipSuccess ||
        hipStreamCreateWithFlags(&ctx->stC, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&ctx->stD, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&ctx->stL[0], hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&ctx->stL[1], hipStreamNonBlocking) != hipSuccess) {
        free_all(ctx);
        delete ctx;
        return HDRF_E_HIP;
    }
    const int B = c.max_batch_blocks;
    ctx->max_batch = B;
    // minimum chunk is window+2 bytes; +2 for the drop-last/append rule and rounding
    ctx->cap_blk = (int)(c.max_block_bytes / (c.window + 2) + 2);
    ctx->ntiles = (ctx->cap_blk + 255) / 256;
    ctx->ev_cap = (int)(B * (c.max_block_bytes / ((int64_t)c.container_max - c.max_chunk) + 2) + 16);
    ctx->closed_cap = 3 * ctx->ev_cap;
    ctx->coll_cap = 1 << 16;
    const size_t nchunk = (size_t)B * ctx->cap_blk;
    for (auto &S : ctx->sl)
        if (!rc) rc = alloc_slot(ctx, S);
    if (!rc && ((rc = dalloc(ctx, &ctx->d_tab, (size_t)1 << c.index_log2)) ||
                (rc = dalloc(ctx, &ctx->d_arena, (size_t)c.arena_slots * c.container_max + 256)) ||
                (rc = dalloc(ctx, &ctx->d_alloc, 1)))) {
    }
    if (!rc && c.compressor == 2) {
        ctx->cslot = lz4_slot_bytes(c.container_max);
        rc = dalloc(ctx, &ctx->d_carena, (size_t)c.arena_slots * ctx->cslot + 256);
    }
    ctx->G = c.n_ranks;
    ctx->rank = c.rank;
    if (!rc && ctx->G > 1) {
        // scratch table for the batch's local aggregation: >= 1.5x the expected distinct chunks
        // (mean chunk ~949 B on random data; a table-full condition is reported, never silent)
        const double expect = 1.5 * (double)B * (double)c.max_block_bytes / 900.0;
        int lg = 16;
        while (lg < 31 && (double)(1ull << lg) < expect) lg++;
        ctx->scratch_log2 = lg;
        ctx->gx_cap = (int64_t)nchunk;
        // batches in the node-global pipeline: the fronts of the next ones (chunking on W, SHA on A,
        // local aggregation on X) run while the oldest goes through its exchanges and back phases
        const char *gd = getenv("HDRF_GX_DEPTH");
        ctx->gx_depth = std::max(2, std::min(kSlots, gd ? atoi(gd) : 3));
        ctx->fn_mcap = gx_fn_mcap(c.container_max, c.window, B);
        ctx->fn_bytes = gx_fn_bytes(c.container_max, c.window, B);
        const size_t nrec = (size_t)ctx->G * (size_t)ctx->gx_cap;
        for (int i = 0; i < ctx->gx_depth && !rc; i++)
            if ((rc = dalloc(ctx, &ctx->d_scratch[i], (size_t)1 << lg)) || (rc = dalloc(ctx, &ctx->d_gxe[i], 64)) ||
                (rc = halloc(ctx, &ctx->sl[i].h_gx, 1))) {
            }
        if (!rc && hipStreamCreateWithFlags(&ctx->stX, hipStreamNonBlocking) != hipSuccess)
            rc = set_err(ctx, HDRF_E_HIP, "hipStreamCreate failed");
        if (!rc && c.timing)
            for (auto &T : ctx->gxt)
                for (auto &e : T.ev)
                    if (!rc && hipEventCreate(&e) != hipSuccess) rc = set_err(ctx, HDRF_E_HIP, "hipEventCreate failed");
        if (rc) {
        } else if ((rc = dalloc(ctx, &ctx->d_x3want, 64)) || (rc = dalloc(ctx, &ctx->d_gxst, 4)) ||
            (rc = dalloc(ctx, &ctx->d_gx_err, 1)) ||
            (rc = dalloc(ctx, &ctx->d_gx_counts, 64)) ||
            (rc = dalloc(ctx, &ctx->d_gx_rcounts, 64)) || (rc = dalloc(ctx, &ctx->d_gx_x3exp, 64)) ||
            (rc = dalloc(ctx, &ctx->d_oslot, nrec)) ||
            (rc = dalloc(ctx, &ctx->d_oflags, nrec))) {
        }
        // owner slots start defined (hdrf_gx_owner's kernels never read a slot the claim did not write
        // once an error is raised, but a defined value keeps any later misuse inside the table)
        if (!rc && (hipMemset(ctx->d_oslot, 0, sizeof(uint32_t) * nrec) != hipSuccess ||
                    hipMemset(ctx->d_gx_err, 0, sizeof(int)) != hipSuccess))
            rc = set_err(ctx, HDRF_E_HIP, "hipMemset failed");
    }
    ctx->timing = c.timing != 0;
    {
        int ncu = 0;
        if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, c.device) == hipSuccess && ncu > 0)
            ctx->n_cu = ncu;
    }
    if (!rc) rc = init_state(ctx, true);
    if (rc) {
        fprintf(stderr, "hdrf_open: %s\n", ctx->err.c_str());
        free_all(ctx);
        delete ctx;
        return rc;
    }
    *out = ctx;
    return 0;
}

extern "C" int hdrf_close(hdrf_ctx *ctx)
{
    if (!ctx) return HDRF_E_INVAL;
    (void)drain(ctx);
    free_all(ctx);
    delete ctx;
    return 0;
}

extern "C" const char *hdrf_last_error(const hdrf_ctx *ctx) { return ctx ? ctx->err.c_str() : "null context"; }
extern "C" int hdrf_digest_len(const hdrf_ctx *ctx) { return ctx ? ctx->H : HDRF_E_INVAL; }

extern "C" int hdrf_reset(hdrf_ctx *ctx)
{
    HDRF_LOCK(ctx);
    if (!ctx) return HDRF_E_INVAL;
    // a receiver may still be appending to a buffer without the lock: refuse rather than race it
    for (int i = 0; i < hdrf_ctx::kRx; i++)
        if (ctx->rx[i].state.load() == 1)
            return set_err(ctx, HDRF_E_INVAL, "a block is being received (hdrf_submit_slot or hdrf_rx_cancel first)");
    return init_state(ctx, false);
}

// A fresh DataNode without draining the pipeline (bench steps back to back, a DataNode's volume
// re-initialised while blocks are in flight): the batches already submitted complete against the
// old state; the next submit starts a new index generation (the next epoch of the tag words, so no
// table clear), the allocator is re-seeded on the index stream after the old batches' store part,
// and the host side (containers, recipes, allocator view, totals) is reset when that batch is
// completed (wait_one), after every older batch.  Single-node contexts.  Durable containers
// (retain_containers): the old generation's containers are drained as its batches complete, before
// the new generation's first batch is waited for (that wait fails otherwise: the new generation
// reuses the container ids); the slot rings continue across the generations, so no slot the old
// generation may still hand out is reopened early.
extern "C" int hdrf_reset_async(hdrf_ctx *ctx)
{
    HDRF_LOCK(ctx);
    if (!ctx) return HDRF_E_INVAL;
    for (int i = 0; i < hdrf_ctx::kRx; i++)
        if (ctx->rx[i].state.load() == 1)
            return set_err(ctx, HDRF_E_INVAL, "a block is being received (hdrf_submit_slot or hdrf_rx_cancel first)");
    if (ctx->G > 1) {
        // node-global: the switch is made by the back phases of the next launched front's batch
        // (hdrf_gx_owner: the next epoch, the node's allocator re-seeded on the back stream after the
        // old batches' commits; hdrf_gx_place_wait: the host side), since the owner phases of the
        // batches in flight are still to be enqueued with the old epoch
        if (ctx->gx_nfront == ctx->gx_nback && !ctx->gen_pending) return init_state(ctx, false);
        ctx->gen_pending = true;
        return 0;
    }
    if (ctx->nsub == ctx->nwait && !ctx->gen_pending) return init_state(ctx, false);   // nothing in flight
    ctx->gen_clear = ctx->gen_clear || ctx->epoch >= 255;
    ctx->epoch = ctx->epoch >= 255 ? 1 : ctx->epoch + 1;
    ctx->bfirst = ctx->batch + 1;
    // durable containers: the new generation continues every slot ring past the old open container
    // (idx_clear_kernel), which stays the old generation's until the switch: one more slot held per
    // switch still in flight (a second hdrf_reset_async before the first switch was waited for holds
    // a second one; calls with no submit in between make one switch)
    if (ctx->cfg.retain_containers && !ctx->gen_pending) ctx->gen_reserve++;
    ctx->gen_pending = true;
    return 0;
}

// container id -> slot bookkeeping after a batch
void host::note_container(hdrf_ctx *ctx, uint32_t id, uint32_t slot, uint32_t len, int closed, uint32_t clen)
{
    auto so = ctx->slot_owner.find(slot);
    if (so != ctx->slot_owner.end() && so->second != id) {
        // durable mode: the ring check in submit() keeps undrained closed containers out of reach
        if (ctx->cfg.retain_containers)
            for (uint32_t u : ctx->pend_closed)
                if (u == so->second) ctx->lost = true;
        ctx->containers.erase(so->second);
    }
    ctx->slot_owner[slot] = id;
    ctx->containers[id] = ContainerInfo{slot, len, closed, clen};
}

ChunkScratch host::chunk_scratch(Slot &S, int compressor)
{
    ChunkScratch X;
    X.ring = compressor == 2 ? 0 : 1;
    X.gm = S.d_gm; X.gstride = S.gstride; X.rq = S.d_rq; X.rq_count = S.d_rq_count; X.rq_cap = (int)S.meta_cap;
    X.rqkeep = S.d_rqkeep;
    X.irr = S.d_irr; X.path = S.d_path; X.jx = S.d_jx; X.jt = S.d_jt; X.jcap = S.jcap; X.wgsum = S.d_wgsum;
    X.maxw = S.maxw_cap;
    return X;
}

// Validate a batch and fill the slot's (pinned) descriptors: the lane segmentation of the chunking
// pass (chunk.hip).  seg_len = segment_bytes / 63 rounded down to a multiple of window + 2, within
// [4, 20] x 702 B.  Grows the slot's speculative lists when needed (the slot's previous batch has
// completed).
int host::prepare_blocks(hdrf_ctx *ctx, Slot &S, int32_t nblocks, const uint8_t *const *dev_data,
                         const uint64_t *len, const uint64_t *readable)
{
    if (nblocks < 1 || nblocks > ctx->max_batch || !dev_data || !len || !readable)
        return set_err(ctx, HDRF_E_INVAL, "bad batch arguments");
    const hdrf_cfg &c = ctx->cfg;
    int64_t max_len = 0;
    for (int b = 0; b < nblocks; b++) {
        if ((int64_t)len[b] > c.max_block_bytes) return set_err(ctx, HDRF_E_INVAL, "block larger than max_block_bytes");
        if (readable[b] < len[b] + kSlack) return set_err(ctx, HDRF_E_INVAL, "readable must be >= len + 64");
        if (((uintptr_t)dev_data[b] & 15) != 0) return set_err(ctx, HDRF_E_INVAL, "block data must be 16-B aligned");
        max_len = std::max(max_len, (int64_t)len[b]);
    }
    S.max_len = max_len;
    const int unit = c.window + 2;
    // one lane per segment: a block of any size has thousands of lanes, so the segment length
    // follows segment_bytes alone (shorter segments only raise the share of boundaries whose
    // chains have not met within the next segment, which then take the repair pass)
    int wins = std::max(kSegMinWin, std::min(kSegMaxWin, (int)(c.segment_bytes / kWaveSegs / unit)));
    // HDRF_SEG_WINS (A/B): the segment length in windows, over segment_bytes
    static const int wins_env = env_int("HDRF_SEG_WINS", 0);
    if (wins_env > 0) wins = std::max(kSegMinWin, std::min(kSegMaxWin, wins_env));
    const int seg_len = wins * unit;
    int seg0 = 0, wave0 = 0;
    for (int b = 0; b < nblocks; b++) {
        BlockDesc &d = S.h_desc[b];
        d.data = dev_data[b];
        d.len = len[b];
        d.readable = readable[b];
        d.nseg = (int)std::max<int64_t>(1, ((int64_t)len[b] + seg_len - 1) / seg_len);
        d.seg_len = seg_len;
        d.seg0 = seg0;
        d.wave0 = wave0;
        seg0 += d.nseg;
        wave0 += (d.nseg + kWaveSegs - 1) / kWaveSegs;
    }
    S.total_waves = wave0;
    S.total_segs = seg0;
    int max_nseg = 1;
    for (int b = 0; b < nblocks; b++) max_nseg = std::max(max_nseg, S.h_desc[b].nseg);
    S.max_nseg = max_nseg;
    const int maxw = (max_nseg + 255) / 256;
    if (maxw > S.maxw_cap) {
        (void)hipFree(S.d_wgsum);
        S.d_wgsum = nullptr;
        S.maxw_cap = 0;
        if (int rc = dalloc(ctx, &S.d_wgsum, (size_t)ctx->max_batch * maxw)) return rc;
        S.maxw_cap = maxw;
    }
    S.spec_cap = lane_spec_cap(seg_len, c.window);
    const size_t words = (size_t)seg0 * S.spec_cap;
    if ((size_t)seg0 > S.meta_cap) {
        (void)hipFree(S.d_meta);
        (void)hipFree(S.d_rq);
        S.d_meta = nullptr;
        S.d_rq = nullptr;
        S.meta_cap = 0;
        if (int rc = dalloc(ctx, &S.d_meta, (size_t)seg0)) return rc;
        if (int rc = dalloc(ctx, &S.d_rq, (size_t)seg0)) return rc;
        (void)hipFree(S.d_irr);
        S.d_irr = nullptr;
        if (int rc = dalloc(ctx, &S.d_irr, (size_t)seg0 / 32 + 2)) return rc;
        S.meta_cap = (size_t)seg0;
    }
    if (words > S.spec_words) {
        (void)hipFree(S.d_spec);
        S.d_spec = nullptr;
        S.spec_words = 0;
        if (int rc = dalloc(ctx, &S.d_spec, words)) return rc;
        S.spec_words = words;
    }
    return 0;
}

StoreParams host::store_params(const hdrf_ctx *ctx, int nblocks)
{
    const hdrf_cfg &c = ctx->cfg;
    StoreParams P;
    P.nblocks = nblocks; P.cap_blk = ctx->cap_blk; P.ntiles = ctx->ntiles;
    P.n_thread = c.n_thread; P.min_mt = c.min_mt_chunks; P.cmax = c.container_max;
    P.nslots = (uint32_t)c.arena_slots; P.ev_cap = ctx->ev_cap; P.closed_cap = ctx->closed_cap;
    return P;
}

// Upper bound on the containers one storer range can close in a batch of `bytes` new bytes: a
// container closes when its length plus the next chunk exceeds container_max, so it holds more
// than container_max - max_chunk - 1 bytes, and two consecutive closes hold more than
// container_max between them (DN/DataDeduplicator.java:748-796).
static uint32_t close_bound(const hdrf_cfg &c, uint64_t bytes)
{
    const uint64_t a = bytes / std::max<uint64_t>(1, (uint64_t)c.container_max - (uint64_t)c.max_chunk - 1);
    const uint64_t b = 2 * bytes / c.container_max;
    return (uint32_t)std::min<uint64_t>(std::min(a, b), 1u << 30) + 1;
}

// The front of a batch, as the single-GPU submit and the node-global front launch both enqueue it:
// the descriptors go up on G (after the packet copies when after_copy), chunking runs on W (its granule
// pass on G), then the fingerprints on A once the walk is done and the recipe copies of the slot's
// previous batch have read d_dig.  mw / ma: the stage markers of W and A.
int host::enqueue_front(hdrf_ctx *ctx, Slot &S, int nblocks, hipStream_t W, hipStream_t G, hipStream_t A, Marker *mw,
                        Marker *ma, bool after_copy)
{
    const hdrf_cfg &c = ctx->cfg;
    if (after_copy) HIPCK(hipStreamWaitEvent(G, S.copy_done, 0));
    HIPCK(hipMemcpyAsync(S.d_blocks, S.h_desc, sizeof(BlockDesc) * nblocks, hipMemcpyHostToDevice, G));
    HIPCK(launch_chunking(S.d_blocks, nblocks, S.max_len, S.max_nseg, S.total_waves, S.total_segs,
                          chunk_scratch(S, c.compressor), c.window, c.max_chunk, S.d_spec, S.spec_cap, S.d_meta, S.d_bst,
                          S.d_off, ctx->cap_blk, S.d_err, W, mw, G, S.gmax_done));
    mw->mark(W);
    HIPCK(hipEventRecord(S.walk_done, W));
    HIPCK(hipStreamWaitEvent(A, S.walk_done, 0));
    if (S.recipe_pending) HIPCK(hipStreamWaitEvent(A, S.recipe_done, 0));
    HIPCK(launch_sha(c.hasher, S.d_blocks, nblocks, S.d_off, S.d_bst, ctx->cap_blk, S.d_dig, S.d_queue, ctx->sha_long, A,
                     ma));
    ma->mark(A);
    return 0;
}

// Enqueue one batch: front on stream A, back on stream B (see the file comment).
int host::submit(hdrf_ctx *ctx, int32_t nblocks, const uint8_t *const *dev_data, const uint64_t *len,
                 const uint64_t *readable, const uint64_t *block_ids, bool after_copy)
{
    if (ctx->nsub - ctx->nwait >= (uint64_t)kSlots)
        if (int rc = wait_one(ctx)) return rc;
    Slot &S = ctx->sl[ctx->nsub % kSlots];
    const hdrf_cfg &c = ctx->cfg;
    if (int rc = prepare_blocks(ctx, S, nblocks, dev_data, len, readable)) return rc;
    S.close_bound = 0;
    if (c.retain_containers) {
        // durable containers: the ring of every storer range (arena_slots / 4 slots, its open
        // container included) must keep room for the closes this batch and the batches in flight
        // can make without reaching an undrained closed container
        uint64_t bytes = 0;
        for (int b = 0; b < nblocks; b++) bytes += len[b];
        const uint32_t bound = close_bound(c, bytes), per = (uint32_t)(c.arena_slots / 4);
        // Only completed batches' containers can be drained: when the batches in flight are part of
        // what fills the ring, the recovery is hdrf_wait_batch (oldest), then hdrf_drain_containers,
        // then the submit again; the message names the step.
        for (int t = 0; t < c.n_thread; t++)
            if ((uint64_t)ctx->undrained[t] + ctx->inflight_bound + ctx->gen_reserve + bound > per - 1)
                return set_err(ctx, HDRF_E_CAPACITY,
                               "container arena: the ring of storer range " + std::to_string(t) + " is full (" +
                                   std::to_string(ctx->undrained[t]) + " undrained closed containers, " +
                                   std::to_string(ctx->inflight_bound) + " closes bounded for batches in flight)" +
                                   (ctx->inflight_bound ? " (hdrf_wait_batch, then hdrf_drain_containers)"
                                                        : " (hdrf_drain_containers first)"));
        S.close_bound = bound;
        ctx->inflight_bound += bound;
    }
    S.ids.assign(nblocks, 0);
    if (block_ids) S.ids.assign(block_ids, block_ids + nblocks);
    S.lens.assign(len, len + nblocks);
    S.nblocks = nblocks;
    S.gen_reset = ctx->gen_pending;                   // the first batch of a fresh generation (hdrf_reset_async)
    ctx->gen_pending = false;
    const uint32_t cur = ++ctx->batch;
    // chunking runs on its own stream W (HDRF_STREAMS=2: shares stream A with SHA).  Measured with
    // the two-pass lane walker (r02): three streams 992 GB/s vs two 919 — the walk's latency-bound
    // kernels and the HBM-bound granule pass overlap SHA's VALU stream of the previous batch
    static const int nstreams = env_int("HDRF_STREAMS", 3);
    hipStream_t W = nstreams == 3 ? ctx->stW : ctx->st, A = ctx->st, Bst = ctx->stB;
    // HDRF_GMAX_STREAM=1: the granule-max pass on stream G, so the next batch's (HBM-bound) pass
    // runs while W walks and stitches this one (latency-bound)
    static const bool gstream = env_int("HDRF_GMAX_STREAM", 0) != 0;
    hipStream_t G = gstream ? ctx->stG : W;
    // ---- chunking on W (the slot's previous batch has completed: wait_one ran, so W may overwrite it),
    // fingerprints on A
    Marker mw, ma;
    mw.ev = ctx->timing ? S.evW : nullptr;
    ma.ev = ctx->timing ? S.evA : nullptr;
    if (int rc = enqueue_front(ctx, S, nblocks, W, G, A, &mw, &ma, after_copy)) return rc;
    HIPCK(hipEventRecord(S.front_done, A));
    // ---- back, index part, in block order on stream B: claim .. decide, then idx_finalize takes the
    // batch-local state out of the index (designated chunks, block counts, entries cleared), so the
    // next batch's index part may run while this batch is stored on stream B2
    HIPCK(hipStreamWaitEvent(Bst, S.front_done, 0));
    if (S.gen_reset) {
        // a fresh generation: the old batches' store part (stream B2: place writes index values, the
        // flush walk the allocator) is finished before this index part claims entries of the new epoch;
        // then the allocator is re-seeded (and the table cleared when the epoch wrapped)
        if (ctx->nsub > ctx->nwait) HIPCK(hipStreamWaitEvent(Bst, ctx->sl[(ctx->nsub - 1) % kSlots].back_done, 0));
        HIPCK(launch_index_clear(ctx->d_tab, ctx->gen_clear ? c.index_log2 : -1, ctx->d_alloc, initial_alloc(ctx), Bst,
                                 c.retain_containers ? (uint32_t)(c.arena_slots / 4) : 0u));
        ctx->gen_clear = false;
    }
    // HDRF_DECIDE_DESIG=0 (A/B): idx_finalize reads every designated entry (round-3 c2 behaviour)
    static const bool decide_desig = env_int("HDRF_DECIDE_DESIG", 1) != 0;
    Marker mb;
    mb.ev = ctx->timing ? S.evB : nullptr;
    HIPCK(launch_index(c.hasher, S.d_bst, nblocks, ctx->cap_blk, S.d_off, S.d_dig, ctx->d_tab, c.index_log2, cur,
                       ctx->bfirst, tag_mask(ctx), S.d_slot, S.d_coll, S.d_ncoll, ctx->coll_cap, S.d_flags, S.d_tilesum, ctx->ntiles,
                       S.d_err, Bst, &mb, decide_desig ? S.d_dcnt : nullptr));
    HIPCK(launch_index_finalize(S.d_bst, nblocks, ctx->cap_blk, ctx->ntiles, ctx->d_tab, S.d_slot, S.d_flags, S.d_dcnt,
                                Bst));
    if (ctx->timing) HIPCK(hipEventRecord(S.evB[9], Bst));
    HIPCK(hipEventRecord(S.idx_done, Bst));
    // ---- back, store part, in block order on stream B2 (scans, flush walk, place, read-back)
    // HDRF_SPLIT_B=0: the store part on stream B too (A/B of the split)
    static const bool split_b = env_int("HDRF_SPLIT_B", 1) != 0;
    hipStream_t B2 = split_b ? ctx->stB2 : Bst;
    HIPCK(hipStreamWaitEvent(B2, S.idx_done, 0));
    HIPCK(hipMemsetAsync(S.d_nclosed, 0, sizeof(uint32_t), B2));
    StoreParams P = store_params(ctx, nblocks);
    // When batches are pipelined (one already in flight), this batch's place kernel overlaps the
    // next batch's front stage (the critical path): a dynamic-LDS reservation caps place at one
    // wave per SIMD so SHA keeps its wave slots (measured +1.5-2% on the config-2 bench; alone,
    // place wants full occupancy).  Under compressor 2 the reservation is 16 KiB: place then fits on
    // a CU as soon as one LZ4 wave of a draining pass leaves it (config 4: 36.96 / 37.01 vs 35.92 /
    // 35.91 GB/s with 40 KiB; 24 KiB 36.5, 9 KiB 36.4; profiles/r02_c4_place_ab.txt).  Round 5, after
    // the LZ4 parse got shorter: 8 KiB 47.31 / 47.27 vs 16 KiB 47.13 / 47.10, 24 KiB 46.68 / 46.74
    // (profiles/r05_c4knobs_ab.txt), so 8 KiB.  HDRF_PLACE_LDS overrides the reservation (bytes).
    static const int place_lds_env = env_int("HDRF_PLACE_LDS", -1);
    const int place_lds = place_lds_env >= 0 ? place_lds_env : (c.compressor == 2 ? 8192 : 40960);
    if (ctx->nsub > ctx->nwait) P.place_lds = place_lds;
    // HDRF_PLACE_DEEP=1: the place copy keeps four 16-B words per thread in flight instead of two
    static const int place_deep_env = env_int("HDRF_PLACE_DEEP", 0);
    P.place_deep = place_deep_env;
    if (c.compressor == 2) {
        // The compression of earlier batches runs on the LZ4 streams, off stream B, so batch k+1's
        // index and store overlap batch k's LZ4 and the LZ4 passes of consecutive batches overlap
        // each other (no per-batch tail on the critical chain).  A place kernel may reopen an arena
        // slot only after the LZ4 pass reading it finished: a slot closed in batch j is reopened
        // at the (arena_slots/4)-th open of its ring after it, and a batch opens at most as many
        // containers per range as it closes (close_bound), so stream B waits for an in-flight
        // batch's LZ4 only when the closes bound from it up to this batch could wrap the ring.
        uint64_t bytes = 0;
        for (int b = 0; b < nblocks; b++) bytes += len[b];
        S.lz_bound = close_bound(c, bytes);
        const uint64_t per = (uint64_t)(c.arena_slots / 4);
        uint64_t sum = S.lz_bound;
        for (uint64_t j = ctx->nsub - 1; j + 1 > ctx->nwait; j--) {   // in flight, newest first
            const Slot &Pj = ctx->sl[j % kSlots];
            sum += Pj.lz_bound;
            // (a fresh generation restarts every ring at its first slot: every pass in flight first)
            if (sum + 1 >= per || S.gen_reset) HIPCK(hipStreamWaitEvent(B2, Pj.lz_done, 0));
            if (j == 0) break;
        }
    }
    HIPCK(launch_store(P, S.d_blocks, S.d_bst, S.d_off, S.d_flags, S.d_tilesum, S.d_tilepre, S.d_store, S.d_pre,
                       ctx->d_alloc, S.d_rstate, S.d_ev, S.d_closed, S.d_nclosed, S.d_slot, ctx->d_tab, ctx->d_arena,
                       S.d_pcid, S.d_ppos, S.d_err, B2, &mb, nullptr, S.d_dcnt));
    if (c.compressor == 2) {    // compression stage: closed containers -> Lz4Codec files (:770-779)
        hipStream_t L = ctx->stL[cur & 1];
        HIPCK(hipEventRecord(S.placed, B2));
        HIPCK(hipStreamWaitEvent(L, S.placed, 0));
        HIPCK(launch_lz4(S.d_closed, S.d_nclosed, ctx->closed_cap, c.container_max, ctx->d_arena, ctx->d_carena,
                         ctx->cslot, S.d_segclen, S.d_filelen, S.d_lzwork, L));
        mb.mark(L);
        HIPCK(hipMemcpyAsync(S.h_filelen, S.d_filelen, sizeof(uint32_t) * ctx->closed_cap, hipMemcpyDeviceToHost, L));
        HIPCK(hipEventRecord(S.lz_done, L));
    } else {
        mb.mark(B2);
    }
    HIPCK(hipMemcpyAsync(S.h_bst, S.d_bst, sizeof(BlockState) * nblocks, hipMemcpyDeviceToHost, B2));
    HIPCK(hipMemcpyAsync(S.h_store, S.d_store, sizeof(uint64_t) * nblocks, hipMemcpyDeviceToHost, B2));
    HIPCK(hipMemcpyAsync(S.h_alloc, ctx->d_alloc, sizeof(AllocState), hipMemcpyDeviceToHost, B2));
    HIPCK(hipMemcpyAsync(S.h_err, S.d_err, sizeof(int), hipMemcpyDeviceToHost, B2));
    HIPCK(hipMemcpyAsync(S.h_nclosed, S.d_nclosed, sizeof(uint32_t), hipMemcpyDeviceToHost, B2));
    HIPCK(hipMemcpyAsync(S.h_long, S.d_queue + 64, sizeof(uint32_t), hipMemcpyDeviceToHost, B2));
    HIPCK(hipMemcpyAsync(S.h_closed, S.d_closed, sizeof(ClosedRec) * ctx->closed_cap, hipMemcpyDeviceToHost, B2));
    HIPCK(hipEventRecord(S.back_done, B2));
    S.pending = true;
    ctx->nsub++;
    return 0;
}

static int complete_state(hdrf_ctx *ctx, Slot &S);

// space for one recipe's digests in the device recipe store (4-B aligned words; entries start
// on 16 B)
int host::recipe_alloc(hdrf_ctx *ctx, uint64_t bytes, uint32_t key, uint32_t n, uint8_t **dst)
{
    constexpr uint64_t kChunk = 256ull << 20;
    if (bytes > kChunk) return set_err(ctx, HDRF_E_CAPACITY, "recipe larger than a recipe-store chunk");
    if (ctx->rcur < ctx->rchunks.size() && ctx->rhead + bytes > kChunk) { ctx->rcur++; ctx->rhead = 0; }
    if (ctx->rcur >= ctx->rchunks.size()) {
        uint8_t *p = nullptr;
        HIPCK(hipMalloc((void **)&p, kChunk));
        ctx->rchunks.push_back(p);
        ctx->rcur = (uint32_t)ctx->rchunks.size() - 1;
        ctx->rhead = 0;
    }
    *dst = ctx->rchunks[ctx->rcur] + ctx->rhead;
    ctx->recipes[key] = hdrf_ctx::RecipeLoc{ctx->rcur, ctx->rhead, n};
    ctx->seeks.erase(key);                           // a seek table describes the recipe it was built from
    ctx->rhead += (bytes + 15) & ~15ull;
    return 0;
}

// GET longToBytes(id,4): [BE32 size | digests] out of the device store; the caller drained.
// 1 found, 0 absent, < 0 error
int host::fetch_recipe(hdrf_ctx *ctx, uint32_t key, std::vector<uint8_t> &r)
{
    auto it = ctx->recipes.find(key);
    if (it == ctx->recipes.end()) return 0;
    const int64_t ln = ctx->lengths[key];
    r.resize(4 + (size_t)it->second.n * ctx->H);
    r[0] = (uint8_t)(ln >> 24); r[1] = (uint8_t)(ln >> 16); r[2] = (uint8_t)(ln >> 8); r[3] = (uint8_t)ln;
    if (it->second.n)
        HIPCK(hipMemcpy(r.data() + 4, ctx->rchunks[it->second.chunk] + it->second.off, (size_t)it->second.n * ctx->H,
                        hipMemcpyDeviceToHost));
    return 1;
}

// After a batch's read-back landed: container / recipe / allocator bookkeeping.
int host::complete_slot(hdrf_ctx *ctx, int si, bool timed)
{
    Slot &S = ctx->sl[si];
    const int nblocks = S.nblocks;
    if (ctx->timing && timed) {
        ctx->stage_ms[11] += elapsed(S.evW[0], S.evW[1]);
        for (int i = 0; i < 2; i++) ctx->stage_ms[i] += elapsed(S.evW[i + 1], S.evW[i + 2]);
        for (int i = 0; i < 2; i++) ctx->stage_ms[2 + i] += elapsed(S.evA[i], S.evA[i + 1]);
        // (evB[9]: the end of the index part on stream B; evB[3..]: the store part on stream B2)
        for (int i = 0; i < 6; i++) ctx->stage_ms[4 + i] += elapsed(S.evB[i], i == 2 ? S.evB[9] : S.evB[i + 1]);
        ctx->stage_ms[10] += elapsed(S.evB[7], S.evB[8]);
    }
    ctx->res = si;
    ctx->last_nblocks = nblocks;
    ctx->probe_stale = false;
    ctx->h_alloc = *S.h_alloc;
    const int herr = *S.h_err;
    if (herr) {
        HIPCK(hipMemsetAsync(S.d_err, 0, sizeof(int), ctx->stB));
        HIPCK(hipStreamSynchronize(ctx->stB));
        *S.h_err = 0;
        return device_error(ctx, herr);
    }
    return complete_state(ctx, S);
}
static int complete_state(hdrf_ctx *ctx, Slot &S)
{
    const hdrf_cfg &c = ctx->cfg;
    const int nblocks = S.nblocks;
    const uint32_t nclosed = *S.h_nclosed;
    ctx->sha_long = *S.h_long != 0;               // long SHA lanes for the next submissions
    if ((int)nclosed > ctx->closed_cap) return set_err(ctx, HDRF_E_CAPACITY, "closed-container list overflow");
    ctx->inflight_bound -= std::min(ctx->inflight_bound, S.close_bound);
    S.close_bound = 0;
    for (uint32_t i = 0; i < nclosed; i++) {
        const ClosedRec &r = S.h_closed[i];
        // (node-global contexts compress after the head pieces are gathered: hdrf_gx_compress)
        const uint32_t flen = c.compressor == 2 && ctx->G == 1 ? S.h_filelen[i] : r.len;
        note_container(ctx, r.id, r.slot, r.len, 1, flen);
        if (c.retain_containers) {
            ctx->pend_closed.push_back(r.id);
            ctx->undrained[std::min<uint32_t>(r.id >> 22, 3)]++;
        }
        ctx->stats.closed_containers++;
        ctx->stats.closed_raw_bytes += r.len;
        ctx->stats.closed_file_bytes += flen;
    }
    for (int t = 0; t < c.n_thread; t++)
        if (ctx->h_alloc.exists[t]) note_container(ctx, ctx->h_alloc.id[t], ctx->h_alloc.slot[t], ctx->h_alloc.cur[t], 0);
    if (ctx->lost) return set_err(ctx, HDRF_E_CAPACITY, "an undrained closed container's arena slot was reused");
    ctx->have_alloc = 1;                              // storeDB always SETs "blockID" (:389)
    for (int b = 0; b < nblocks; b++) {
        ctx->stats.blocks++;
        ctx->stats.logical_bytes += S.lens[b];
        ctx->stats.new_bytes += S.h_store[b];
        ctx->stats.chunks += S.h_bst[b].n_chunks;
        ctx->stats.recipe_bytes += 4 + (uint64_t)S.h_bst[b].n_chunks * ctx->H;
    }
    ctx->stats.open_bytes = 0;
    for (int t = 0; t < c.n_thread; t++)
        if (ctx->h_alloc.exists[t]) ctx->stats.open_bytes += ctx->h_alloc.cur[t];
    // recipes (SET longToBytes(id,4) -> BE32 size | digests): the block's digests are copied on
    // the device into the recipe store off stream B (the critical chain): on stream C, or on stream R
    // once host batches put H2D copies on C (a recipe kernel there held back the copies queued behind
    // it).  R exists only then: one more stream from the open on changed how the hardware queues are
    // shared and config 4's two LZ4 passes stopped overlapping (40.5 -> 34.2 GB/s,
    // profiles/r04_c4_stream_ab.txt).  The slot's next SHA waits for the copies.
    int nj = 0;
    for (int b = 0; b < nblocks; b++) {
        const uint32_t key = (uint32_t)S.ids[b];
        ctx->lengths[key] = (int64_t)S.lens[b];
        if (c.keep_recipes) {
            const uint32_t n = (uint32_t)S.h_bst[b].n_chunks;
            uint8_t *dst = nullptr;
            if (int rc = recipe_alloc(ctx, (uint64_t)n * ctx->H, key, n, &dst)) return rc;
            S.h_rjobs[nj++] = RecipeCopy{(uint64_t)(uintptr_t)(S.d_dig + (size_t)b * ctx->cap_blk * ctx->HW),
                                         (uint64_t)(uintptr_t)dst, n * (uint32_t)ctx->HW, 0};
        }
    }
    if (nj) {
        if (ctx->host_copies && !ctx->stR) HIPCK(hipStreamCreateWithFlags(&ctx->stR, hipStreamNonBlocking));
        hipStream_t rs = ctx->host_copies ? ctx->stR : ctx->stC;
        HIPCK(hipMemcpyAsync(S.d_rjobs, S.h_rjobs, sizeof(RecipeCopy) * nj, hipMemcpyHostToDevice, rs));
        HIPCK(launch_recipe_copy(S.d_rjobs, nj, rs));
        HIPCK(hipEventRecord(S.recipe_done, rs));
        S.recipe_pending = true;
    }
    return 0;
}


// Durable containers: is any container of the current host generation not yet handed out (closed
// ones, and the bytes of the open ones)?  A new generation reuses their ids.
static bool gen_undrained(const hdrf_ctx *ctx)
{
    if (!ctx->pend_closed.empty()) return true;
    for (int t = 0; t < ctx->cfg.n_thread && ctx->have_alloc; t++) {
        if (!ctx->h_alloc.exists[t]) continue;
        auto it = ctx->containers.find(ctx->h_alloc.id[t]);
        auto h = ctx->handed.find(ctx->h_alloc.id[t]);
        const int64_t done = h != ctx->handed.end() ? h->second : 0;
        if (it != ctx->containers.end() && (int64_t)it->second.len > done) return true;
    }
    return false;
}

// Complete the oldest batch in flight (its slot is reusable once this returns).  The first batch of
// a fresh generation (hdrf_reset_async) on a durable context is refused while the old generation's
// containers are not drained, and stays in flight: hdrf_drain_containers, then hdrf_wait_batch again.
// force (drain(): a view, a reset or close): it completes anyway and the context is marked lost.
static int wait_one(hdrf_ctx *ctx, bool force)
{
    if (ctx->nwait >= ctx->nsub) return set_err(ctx, HDRF_E_INVAL, "no batch in flight");
    const int si = (int)(ctx->nwait % kSlots);
    Slot &S = ctx->sl[si];
    const bool refused = S.gen_reset && ctx->cfg.retain_containers && gen_undrained(ctx);
    if (refused && !force)
        return set_err(ctx, HDRF_E_INVAL, "hdrf_reset_async: the previous generation's containers were not "
                                          "drained before its successor's first batch was waited for "
                                          "(hdrf_drain_containers, then hdrf_wait_batch again)");
    ctx->nwait++;
    S.pending = false;
    HIPCK(hipEventSynchronize(S.back_done));
    if (ctx->cfg.compressor == 2) HIPCK(hipEventSynchronize(S.lz_done));
    for (int i = 0; i < hdrf_ctx::kRx; i++)            // its receive buffers are free again
        if (S.rx_release >> i & 1) {
            ctx->rx[i].state = 0;
            ctx->rx[i].len = 0;
        }
    S.rx_release = 0;
    if (S.gen_reset) {                                   // the first batch of a fresh generation
        if (ctx->cfg.retain_containers) {
            ctx->handed.clear();
            // this switch's ring continuation is over (one per pending durable generation switch)
            ctx->gen_reserve -= std::min<uint32_t>(ctx->gen_reserve, 1u);
        }
        reset_host(ctx);
        S.gen_reset = false;
        if (refused) {
            ctx->lost = true;
            (void)complete_slot(ctx, si, true);
            return set_err(ctx, HDRF_E_CAPACITY, "hdrf_reset_async: the previous generation's undrained containers "
                                                 "were dropped (the context needs hdrf_reset)");
        }
    }
    return complete_slot(ctx, si, true);
}

extern "C" int hdrf_submit_batch(hdrf_ctx *ctx, int32_t nblocks, const uint8_t *const *dev_data, const uint64_t *len,
                                 const uint64_t *readable, const uint64_t *block_ids)
{
    HDRF_LOCK(ctx);
    if (!ctx) return HDRF_E_INVAL;
    if (ctx->G > 1) return set_err(ctx, HDRF_E_INVAL, "node-global context: use the hdrf_gx_* phases");
    if (ctx->nsub - ctx->nwait >= (uint64_t)kSlots)     // every submit pairs with one hdrf_wait_batch
        return set_err(ctx, HDRF_E_CAPACITY, "pipeline full: hdrf_wait_batch first");
    return submit(ctx, nblocks, dev_data, len, readable, block_ids);
}

// Host-resident batch: the blocks are copied into the slot's device staging buffer on stream C
// (hipMemcpyAsync; overlapped with the kernels of the batches in flight when the host memory is
// pinned), then reduced exactly like hdrf_submit_batch.
extern "C" int hdrf_submit_host(hdrf_ctx *ctx, int32_t nblocks, const uint8_t *const *host_data, const uint64_t *len,
                                const uint64_t *block_ids)
{
    HDRF_LOCK(ctx);
    if (!ctx) return HDRF_E_INVAL;
    if (ctx->G > 1) return set_err(ctx, HDRF_E_INVAL, "node-global context: use the hdrf_gx_* phases");
    if (nblocks < 1 || nblocks > ctx->max_batch || !host_data || !len) return set_err(ctx, HDRF_E_INVAL, "bad batch arguments");
    for (int b = 0; b < nblocks; b++) {
        if ((int64_t)len[b] > ctx->cfg.max_block_bytes) return set_err(ctx, HDRF_E_INVAL, "block larger than max_block_bytes");
        if (len[b] && !host_data[b]) return set_err(ctx, HDRF_E_INVAL, "null block data");
    }
    if (ctx->nsub - ctx->nwait >= (uint64_t)kSlots)     // every submit pairs with one hdrf_wait_batch
        return set_err(ctx, HDRF_E_CAPACITY, "pipeline full: hdrf_wait_batch first");
    Slot &S = ctx->sl[ctx->nsub % kSlots];
    ctx->host_copies = true;
    const uint64_t stride = ((uint64_t)ctx->cfg.max_block_bytes + kSlack + 255) & ~(uint64_t)255;
    if (!S.d_hstage) {                                 // first host batch of this slot
        HIPCK(hipMalloc((void **)&S.d_hstage, stride * ctx->max_batch));
        S.hstage_stride = stride;
    }
    std::vector<const uint8_t *> ptrs(nblocks);
    std::vector<uint64_t> rd(nblocks);
    for (int b = 0; b < nblocks; b++) {
        uint8_t *d = S.d_hstage + (uint64_t)b * stride;
        // Only the copies go on stream C.  The 64 readable bytes past the block end are not filled:
        // the kernels never depend on them (device batches hand over arbitrary bytes there, e.g. the
        // next block), and a fill kernel between the copies waited for CU slots behind the drain and
        // the reduction, stalling the copy engine 8-10 ms per 16-block batch (config 5 trace, r04).
        if (len[b]) HIPCK(hipMemcpyAsync(d, host_data[b], len[b], hipMemcpyHostToDevice, ctx->stC));
        ptrs[b] = d;
        rd[b] = stride * (uint64_t)(ctx->max_batch - b);
    }
    HIPCK(hipEventRecord(S.copy_done, ctx->stC));
    return submit(ctx, nblocks, ptrs.data(), len, rd.data(), block_ids, true);
}

extern "C" int hdrf_host_alloc(hdrf_ctx *ctx, uint64_t bytes, void **out)
{
    HDRF_LOCK(ctx);
    if (!ctx || !out) return HDRF_E_INVAL;
    HIPCK(hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault));
    return 0;
}

extern "C" int hdrf_host_free(hdrf_ctx *ctx, void *p)
{
    HDRF_LOCK(ctx);
    if (!ctx) return HDRF_E_INVAL;
    if (p) HIPCK(hipHostFree(p));
    return 0;
}

extern "C" int hdrf_wait_batch(hdrf_ctx *ctx)
{
    if (!ctx) return HDRF_E_INVAL;
    // Block on the oldest batch's completion events WITHOUT the context lock, so receiver threads
    // (hdrf_rx_begin, hdrf_submit_slot) and drains are not stalled behind a GPU wait; wait_one then
    // finds the events complete.  (Should the slot be waited and reused meanwhile, its events
    // belong to a newer batch: this only waits longer.)
    hipEvent_t ev[2] = {nullptr, nullptr};
    {
        HDRF_LOCK(ctx);
        if (ctx->nwait < ctx->nsub) {
            const Slot &S = ctx->sl[(int)(ctx->nwait % kSlots)];
            ev[0] = S.back_done;
            if (ctx->cfg.compressor == 2) ev[1] = S.lz_done;
        }
    }
    for (hipEvent_t e : ev)
        if (e) (void)hipEventSynchronize(e);           // errors are reported by wait_one below
    HDRF_LOCK(ctx);
    return wait_one(ctx);
}

extern "C" int hdrf_batch_nblocks(hdrf_ctx *ctx)
{
    HDRF_LOCK(ctx);
    return ctx ? ctx->last_nblocks : HDRF_E_INVAL;
}

extern "C" int hdrf_reduce_batch(hdrf_ctx *ctx, int32_t nblocks, const uint8_t *const *dev_data, const uint64_t *len,
                                 const uint64_t *readable, const uint64_t *block_ids)
{
    HDRF_LOCK(ctx);
    if (!ctx) return HDRF_E_INVAL;
    if (ctx->G > 1) return set_err(ctx, HDRF_E_INVAL, "node-global context: use the hdrf_gx_* phases");
    if (int rc = drain(ctx)) return rc;
    if (int rc = submit(ctx, nblocks, dev_data, len, readable, block_ids)) return rc;
    return wait_one(ctx);
}

static int check_b(hdrf_ctx *ctx, int32_t b)
{
    if (!ctx) return HDRF_E_INVAL;
    if (b < 0 || b >= ctx->last_nblocks) return set_err(ctx, HDRF_E_INVAL, "block index out of range");
    return 0;
}

extern "C" int hdrf_batch_info(hdrf_ctx *ctx, int32_t b, int64_t *n_chunks, int64_t *store_size)
{
    HDRF_LOCK(ctx);
    if (int rc = check_b(ctx, b)) return rc;
    const Slot &R = ctx->sl[ctx->res];
    if (n_chunks) *n_chunks = R.h_bst[b].n_chunks;
    if (store_size) *store_size = (int64_t)R.h_store[b];
    return 0;
}

extern "C" int hdrf_batch_offsets(hdrf_ctx *ctx, int32_t b, uint32_t *out, int64_t cap)
{
    HDRF_LOCK(ctx);
    if (int rc = check_b(ctx, b)) return rc;
    const Slot &R = ctx->sl[ctx->res];
    const int64_t n = R.h_bst[b].n_chunks;
    if (cap < n) return set_err(ctx, HDRF_E_CAPACITY, "offsets capacity");
    HIPCK(hipMemcpy(out, R.d_off + (size_t)b * ctx->cap_blk, n * 4, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int hdrf_batch_digests(hdrf_ctx *ctx, int32_t b, uint8_t *out, int64_t cap_bytes)
{
    HDRF_LOCK(ctx);
    if (int rc = check_b(ctx, b)) return rc;
    const Slot &R = ctx->sl[ctx->res];
    const int64_t n = R.h_bst[b].n_chunks;
    if (cap_bytes < n * ctx->H) return set_err(ctx, HDRF_E_CAPACITY, "digest capacity");
    HIPCK(hipMemcpy(out, R.d_dig + (size_t)b * ctx->cap_blk * ctx->HW, n * ctx->H, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int hdrf_batch_is_new(hdrf_ctx *ctx, int32_t b, uint8_t *out, int64_t cap)
{
    HDRF_LOCK(ctx);
    if (int rc = check_b(ctx, b)) return rc;
    const Slot &R = ctx->sl[ctx->res];
    const int64_t n = R.h_bst[b].n_chunks;
    if (cap < n) return set_err(ctx, HDRF_E_CAPACITY, "is_new capacity");
    HIPCK(hipMemcpy(out, R.d_flags + (size_t)b * ctx->cap_blk, n, hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < n; i++) out[i] &= 1;
    return 0;
}

extern "C" int hdrf_batch_placement(hdrf_ctx *ctx, int32_t b, uint32_t *cid, uint32_t *pos, int64_t cap)
{
    HDRF_LOCK(ctx);
    if (int rc = check_b(ctx, b)) return rc;
    const Slot &R = ctx->sl[ctx->res];
    const int64_t n = R.h_bst[b].n_chunks;
    if (cap < n) return set_err(ctx, HDRF_E_CAPACITY, "placement capacity");
    std::vector<uint8_t> f(n);
    HIPCK(hipMemcpy(f.data(), R.d_flags + (size_t)b * ctx->cap_blk, n, hipMemcpyDeviceToHost));
    if (cid) HIPCK(hipMemcpy(cid, R.d_pcid + (size_t)b * ctx->cap_blk, n * 4, hipMemcpyDeviceToHost));
    if (pos) HIPCK(hipMemcpy(pos, R.d_ppos + (size_t)b * ctx->cap_blk, n * 4, hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < n; i++)
        if (!(f[i] & 1)) {
            if (cid) cid[i] = 0;
            if (pos) pos[i] = 0;
        }
    return 0;
}

// Test hook: the chunker's per-segment records of block b, as the batch's kernels left them in the
// slot (d_meta is written by the lane walk, the repair and the stitch of the slot's own batch only,
// and the next submit to the slot waits for this batch first: the same window as d_off above).
extern "C" int hdrf_batch_seg_trace(hdrf_ctx *ctx, int32_t b, hdrf_seg_trace *out, int64_t cap, int32_t *rq_count)
{
    HDRF_LOCK(ctx);
    if (int rc = check_b(ctx, b)) return rc;
    if (ctx->G > 1) return set_err(ctx, HDRF_E_UNSUPPORTED, "segment trace on node-global contexts");
    if (!out) return set_err(ctx, HDRF_E_INVAL, "null trace buffer");
    const Slot &R = ctx->sl[ctx->res];
    const BlockDesc &d = R.h_desc[b];
    if (cap < d.nseg) return set_err(ctx, HDRF_E_CAPACITY, "segment trace capacity");
    std::vector<SegMeta> m((size_t)d.nseg);
    HIPCK(hipMemcpy(m.data(), R.d_meta + d.seg0, sizeof(SegMeta) * m.size(), hipMemcpyDeviceToHost));
    for (int k = 0; k < d.nseg; k++) {
        const SegMeta &s = m[(size_t)k];
        out[k] = hdrf_seg_trace{s.n_main, s.n_over, s.sync, s.jmp, s.jj, s.n_ext, s.ext_dst, s.pad[0]};
    }
    if (rq_count) HIPCK(hipMemcpy(rq_count, R.d_rq_count, sizeof(int32_t), hipMemcpyDeviceToHost));
    return d.nseg;
}

extern "C" int hdrf_reduce_block(hdrf_ctx *ctx, uint64_t block_id, const uint8_t *data, uint64_t len,
                                 hdrf_block_result *out)
{
    HDRF_LOCK(ctx);
    if (!ctx) return HDRF_E_INVAL;
    if (ctx->G > 1) return set_err(ctx, HDRF_E_INVAL, "node-global context: use the hdrf_gx_* phases");
    if ((int64_t)len > ctx->cfg.max_block_bytes) return set_err(ctx, HDRF_E_INVAL, "block larger than max_block_bytes");
    if (len && !data) return set_err(ctx, HDRF_E_INVAL, "null data");
    const uint64_t need = len + 4096;
    if (ctx->stage_cap < need) {
        if (ctx->d_stage) (void)hipFree(ctx->d_stage);
        ctx->d_stage = nullptr;
        ctx->stage_cap = 0;
        const uint64_t cap = std::max<uint64_t>(need, (uint64_t)ctx->cfg.max_block_bytes + 4096);
        HIPCK(hipMalloc((void **)&ctx->d_stage, cap));
        ctx->stage_cap = cap;
    }
    if (len) HIPCK(hipMemcpyAsync(ctx->d_stage, data, len, hipMemcpyHostToDevice, ctx->st));
    HIPCK(hipMemsetAsync(ctx->d_stage + len, 0, 64, ctx->st));
    const uint8_t *p = ctx->d_stage;
    const uint64_t readable = ctx->stage_cap;
    int rc = hdrf_reduce_batch(ctx, 1, &p, &len, &readable, &block_id);
    if (rc) return rc;
    if (out) {
        int64_t n = 0, ss = 0;
        hdrf_batch_info(ctx, 0, &n, &ss);
        out->n_chunks = n;
        out->store_size = ss;
        if (out->capacity < n && (out->offsets || out->digests || out->is_new || out->container_id || out->container_pos))
            return set_err(ctx, HDRF_E_CAPACITY, "result capacity too small");
        if (out->offsets && (rc = hdrf_batch_offsets(ctx, 0, out->offsets, out->capacity))) return rc;
        if (out->digests && (rc = hdrf_batch_digests(ctx, 0, out->digests, out->capacity * ctx->H))) return rc;
        if (out->is_new && (rc = hdrf_batch_is_new(ctx, 0, out->is_new, out->capacity))) return rc;
        if ((out->container_id || out->container_pos) &&
            (rc = hdrf_batch_placement(ctx, 0, out->container_id, out->container_pos, out->capacity)))
            return rc;
    }
    return 0;
}

// ---- arrival tickets: the FIFO of DN/DataDeduplicator.java:124-158 (DN/DDRunner.java:20-36) ------
extern "C" int hdrf_ticket_take(hdrf_ctx *ctx, uint64_t *ticket)
{
    HDRF_LOCK(ctx);
    if (!ctx || !ticket) return HDRF_E_INVAL;
    *ticket = ctx->next_ticket++;
    return 0;
}

static void ticket_done(hdrf_ctx *ctx, uint64_t ticket)
{
    if (ctx->serving == ticket) {
        ctx->serving++;
        while (ctx->cancelled.count(ctx->serving)) ctx->cancelled.erase(ctx->serving++);
    } else if (ticket > ctx->serving) {
        ctx->cancelled.insert(ticket);
    }
    ctx->turn.notify_all();
}

extern "C" int hdrf_ticket_cancel(hdrf_ctx *ctx, uint64_t ticket)
{
    HDRF_LOCK(ctx);
    if (!ctx || ticket >= ctx->next_ticket) return HDRF_E_INVAL;
    ticket_done(ctx, ticket);
    return 0;
}

extern "C" int hdrf_reduce_block_ticketed(hdrf_ctx *ctx, uint64_t ticket, uint64_t block_id, const uint8_t *data,
                                          uint64_t len, hdrf_block_result *out)
{
    if (!ctx) return HDRF_E_INVAL;
    std::unique_lock<std::recursive_mutex> lk(ctx->mu);
    if (ticket >= ctx->next_ticket || ticket < ctx->serving || ctx->cancelled.count(ticket))
        return set_err(ctx, HDRF_E_INVAL, "unknown or finished ticket");
    ctx->turn.wait(lk, [&] { return ctx->serving == ticket; });
    const int rc = hdrf_reduce_block(ctx, block_id, data, len, out);
    ticket_done(ctx, ticket);
    return rc;
}

// ---- memory helpers, corpus, timing ------------------------------------------------------
extern "C" int hdrf_dev_alloc(hdrf_ctx *ctx, uint64_t bytes, void **out)
{
    HDRF_LOCK(ctx);
    if (!ctx || !out) return HDRF_E_INVAL;
    HIPCK(hipMalloc(out, bytes));
    return 0;
}

extern "C" int hdrf_dev_free(hdrf_ctx *ctx, void *p)
{
    HDRF_LOCK(ctx);
    if (!ctx) return HDRF_E_INVAL;
    if (int rc = drain(ctx)) return rc;
    HIPCK(hipFree(p));
    return 0;
}

extern "C" int hdrf_memcpy_h2d(hdrf_ctx *ctx, void *dst, const void *src, uint64_t bytes)
{
    HDRF_LOCK(ctx);
    if (!ctx) return HDRF_E_INVAL;
    HIPCK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->st));
    HIPCK(hipStreamSynchronize(ctx->st));
    return 0;
}

extern "C" int hdrf_memcpy_d2h(hdrf_ctx *ctx, void *dst, const void *src, uint64_t bytes)
{
    HDRF_LOCK(ctx);
    if (!ctx) return HDRF_E_INVAL;
    HIPCK(hipStreamSynchronize(ctx->st));
    HIPCK(hipStreamSynchronize(ctx->stB));
    HIPCK(hipStreamSynchronize(ctx->stB2));
    HIPCK(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int hdrf_synchronize(hdrf_ctx *ctx)
{
    HDRF_LOCK(ctx);
    if (!ctx) return HDRF_E_INVAL;
    return drain(ctx);                                 // completes every batch in flight
}

extern "C" int hdrf_corpus_fill(hdrf_ctx *ctx, uint8_t *dev, const uint32_t *roots_host, int64_t nblocks,
                                int64_t segs_per_block, int64_t seg_bytes, uint64_t seed)
{
    HDRF_LOCK(ctx);
    return hdrf_corpus_fill_kind(ctx, dev, roots_host, nblocks, segs_per_block, seg_bytes, seed, 0);
}

extern "C" int hdrf_corpus_fill_kind(hdrf_ctx *ctx, uint8_t *dev, const uint32_t *roots_host, int64_t nblocks,
                                     int64_t segs_per_block, int64_t seg_bytes, uint64_t seed, int32_t mixed)
{
    HDRF_LOCK(ctx);
    if (!ctx || !dev || !roots_host || seg_bytes % 16 != 0) return HDRF_E_INVAL;
    uint32_t *d_roots = nullptr;
    const size_t n = (size_t)nblocks * segs_per_block;
    HIPCK(hipMalloc((void **)&d_roots, n * 4));
    HIPCK(hipMemcpyAsync(d_roots, roots_host, n * 4, hipMemcpyHostToDevice, ctx->st));
    HIPCK(launch_corpus(dev, d_roots, nblocks, segs_per_block, seg_bytes, seed, mixed ? 1 : 0, ctx->st));
    HIPCK(hipStreamSynchronize(ctx->st));
    HIPCK(hipFree(d_roots));
    return 0;
}

extern "C" int hdrf_get_stats(hdrf_ctx *ctx, hdrf_stats *out)
{
    HDRF_LOCK(ctx);
    if (!ctx || !out) return HDRF_E_INVAL;
    *out = ctx->stats;
    return 0;
}

extern "C" int hdrf_stage_times(hdrf_ctx *ctx, double *ms, int32_t n, int32_t reset)
{
    HDRF_LOCK(ctx);
    if (!ctx) return HDRF_E_INVAL;
    for (int i = 0; i < n && i < kStages; i++) ms[i] = ctx->stage_ms[i];
    if (reset)
        for (double &v : ctx->stage_ms) v = 0;
    return 0;
}
