// api_gx.hip — libhdrf C-ABI: every hdrf_gx_* entry point, the phases of the node-global index
// (cfg.n_ranks > 1) and its read side.
//
// Writes the gx_* fields of the context (phase counters, allocator exchange, timing ring), the batch
// id and scratch epochs, the slots of its own pipeline (sl[0 .. gx_depth)), and, where a pending
// hdrf_reset_async takes effect (hdrf_gx_owner, hdrf_gx_place_wait), epoch / bfirst / h_alloc and the
// host side through reset_host.  A batch's completion goes through complete_slot (api.hip).
#include "ctx.hpp"

// ---- node-global index phases (include/hdrf.h, gx.hip) ------------------------------------
static_assert(sizeof(AllocState) <= HDRF_ALLOC_STATE_BYTES, "allocator state exchange size");

// back phases run on the oldest batch whose front was waited, in order owner..commit
static int gx_check(hdrf_ctx *ctx, int bphase)
{
    if (!ctx) return HDRF_E_INVAL;
    if (ctx->G < 2) return set_err(ctx, HDRF_E_INVAL, "hdrf_gx_* needs cfg.n_ranks > 1");
    if (ctx->gx_nfwait <= ctx->gx_nback || ctx->gx_bphase != bphase)
        return set_err(ctx, HDRF_E_INVAL, "hdrf_gx_* phases called out of order (back phase " +
                                              std::to_string(ctx->gx_bphase) + ")");
    return 0;
}

static int64_t max_count(const int64_t *counts, int G)
{
    int64_t m = 0;
    for (int i = 0; i < G; i++) m = std::max(m, counts[i]);
    return m;
}

extern "C" int hdrf_gx_layout_get(hdrf_ctx *ctx, hdrf_gx_layout *out)
{
    HDRF_LOCK(ctx);
    if (!ctx || !out) return HDRF_E_INVAL;
    out->cap = ctx->gx_cap;
    out->x1_words = ctx->HW + 2;
    out->x2_words = 2;
    out->x3_words = 4;
    out->depth = ctx->gx_depth;
    out->fn_bytes = (int64_t)ctx->fn_bytes;
    return 0;
}

// ---- node-global pipeline ----------------------------------------------------
// A batch's front half runs like the single-node pipeline: chunking on stream W, SHA on stream A,
// then the local aggregation and its X1 records on stream X, in slot seq % gx_depth, so the fronts
// of the next batches run while the oldest batch goes through its exchanges and back phases on
// stream B.  The back half enqueues without host round trips: the allocator scan runs on the
// device (hdrf_gx_flush_fn_dev -> all-gather of fixed-size descriptors -> hdrf_gx_alloc_scan_dev),
// placement and its read-back are one event the host waits for (the X3 counts size the X3
// exchange), the arena copy runs on stream B2 beside the next batch's owner phases, and the commit
// is not waited for (its errors are reported by the next place or hdrf_gx_sync).

static void gx_mark(hdrf_ctx *ctx, uint64_t seq, int e, hipStream_t st)
{
    if (!ctx->timing) return;
    GxTime &T = ctx->gxt[seq % kGxRing];
    if (hipEventRecord(T.ev[e], st) == hipSuccess) T.rec |= 1u << e;
}

// phase times of completed batches, in order (wait: block until they are complete)
static void gx_collect(hdrf_ctx *ctx, bool wait, uint64_t upto)
{
    if (!ctx->timing) return;
    while (ctx->gxt_done < upto && ctx->gxt_done < ctx->gx_nback) {
        const uint64_t k = ctx->gxt_done;
        GxTime &T = ctx->gxt[k % kGxRing];
        const auto has = [&](int e) { return (T.rec >> e & 1) != 0; };
        for (int e : {(int)kG13, (int)kP1})
            if (has(e)) {
                if (wait) (void)hipEventSynchronize(T.ev[e]);
                else if (hipEventQuery(T.ev[e]) != hipSuccess) return;
            }
        const auto add = [&](int stage, int a, int b) {
            if (has(a) && has(b)) ctx->stage_ms[stage] += elapsed(T.ev[a], T.ev[b]);
        };
        add(11, kW0, kW0 + 1); add(0, kW0 + 1, kW0 + 2); add(1, kW0 + 2, kW0 + 3);
        add(2, kA0, kA0 + 1);
        add(12, kX0, kX0 + 3);
        add(13, kG0, kG1); add(20, kG1, kG2); add(14, kG2, kG3); add(7, kG3, kG4);
        add(15, kG5, kG6); add(21, kG6, kG7); add(16, kG7, kG8); add(8, kG8, kG9);
        add(17, kG10, kG11); add(22, kG11, kG12); add(18, kG12, kG13);
        add(9, kP0, kP1);
        if (k > 0) {                                    // X1 + host gap: the previous commit to this owner phase
            GxTime &Pv = ctx->gxt[(k - 1) % kGxRing];
            if ((Pv.rec >> kG13 & 1) && has(kG0)) ctx->stage_ms[19] += elapsed(Pv.ev[kG13], T.ev[kG0]);
        }
        ctx->gxt_done++;
    }
}

// Front half of a node-global batch (chunking, SHA, local aggregation, X1 records), launched into
// slot nfront % gx_depth without waiting.  The slot's previous batch must have left it: its back
// phases (stream B) and its arena copy (stream B2) are waited for on the device.
extern "C" int hdrf_gx_front_launch(hdrf_ctx *ctx, int32_t nblocks, const uint8_t *const *dev_data, const uint64_t *len,
                                    const uint64_t *readable, const uint64_t *block_ids, uint32_t gbase,
                                    uint32_t *x1_send)
{
    HDRF_LOCK(ctx);
    if (!ctx) return HDRF_E_INVAL;
    if (ctx->G < 2) return set_err(ctx, HDRF_E_INVAL, "hdrf_gx_* needs cfg.n_ranks > 1");
    const uint64_t D = (uint64_t)ctx->gx_depth;
    if (ctx->gx_nfront - ctx->gx_nback >= D)
        return set_err(ctx, HDRF_E_INVAL, "hdrf_gx_front_launch: " + std::to_string(D) +
                                              " batches in the node-global pipeline (commit the oldest first)");
    if (!x1_send) return set_err(ctx, HDRF_E_INVAL, "null exchange buffer");
    const uint64_t seq = ctx->gx_nfront;
    const int si = (int)(seq % D);
    Slot &S = ctx->sl[si];
    const hdrf_cfg &c = ctx->cfg;
    // the timing ring entry is reused: the batch kGxRing - 1 back (and everything before) is collected
    if (ctx->timing) {
        if (seq + 2 > (uint64_t)kGxRing) gx_collect(ctx, true, seq + 2 - kGxRing);
        ctx->gxt[seq % kGxRing].rec = 0;
    }
    hipStream_t W = ctx->stW, A = ctx->st, X = ctx->stX;
    if (S.gx_inuse) {                                   // the slot's previous batch is done with it
        HIPCK(hipStreamWaitEvent(W, S.back_done, 0));
        if (S.gx_split) HIPCK(hipStreamWaitEvent(W, S.placed, 0));
    }
    if (int rc = prepare_blocks(ctx, S, nblocks, dev_data, len, readable)) return rc;
    S.gx_batch = ++ctx->batch;
    GxTime &T = ctx->gxt[seq % kGxRing];
    Marker mw, ma, mx;
    mw.ev = ctx->timing ? &T.ev[kW0] : nullptr;
    ma.ev = ctx->timing ? &T.ev[kA0] : nullptr;
    if (int rc = enqueue_front(ctx, S, nblocks, W, W, A, &mw, &ma)) return rc;
    HIPCK(hipEventRecord(S.idx_done, A));               // (node-global: "the batch's digests are ready")
    // local aggregation: a fresh scratch table (the next epoch of the slot's table, cleared every 255
    // uses), every entry "created" in batch 1
    HIPCK(hipStreamWaitEvent(X, S.idx_done, 0));
    if (++ctx->scratch_epoch[si] > 255) {
        HIPCK(hipMemsetAsync(ctx->d_scratch[si], 0, sizeof(IndexEntry) << ctx->scratch_log2, X));
        ctx->scratch_epoch[si] = 1;
    }
    const unsigned long long skey = ((unsigned long long)ctx->scratch_epoch[si] << 56) | tag_bits(ctx);
    mx.ev = ctx->timing ? &T.ev[kX0] : nullptr;
    HIPCK(launch_index(c.hasher, S.d_bst, nblocks, ctx->cap_blk, S.d_off, S.d_dig, ctx->d_scratch[si],
                       ctx->scratch_log2, 1u, 1u, skey, S.d_slot, S.d_coll, S.d_ncoll, ctx->coll_cap,
                       S.d_flags, S.d_tilesum, ctx->ntiles, S.d_err, X, &mx));
    HIPCK(launch_gx_emit(c.hasher, S.d_bst, nblocks, ctx->cap_blk, ctx->ntiles, S.d_dig, ctx->d_scratch[si],
                         S.d_slot, S.d_flags, gbase, ctx->G, x1_send, ctx->gx_cap, ctx->d_gxe[si], S.d_err, X));
    mx.mark(X);
    HIPCK(hipMemcpyAsync(S.h_gx->front_cnt, ctx->d_gxe[si], sizeof(unsigned long long) * ctx->G, hipMemcpyDeviceToHost, X));
    HIPCK(hipMemcpyAsync(&S.h_gx->front_err, S.d_err, sizeof(int), hipMemcpyDeviceToHost, X));
    HIPCK(hipEventRecord(S.front_done, X));
    if (ctx->timing) T.rec |= 0xFu << kW0 | 0x7u << kA0 | 0xFu << kX0;
    S.nblocks = nblocks;
    S.lens.assign(len, len + nblocks);
    S.ids.assign(nblocks, 0);
    if (block_ids) S.ids.assign(block_ids, block_ids + nblocks);
    S.gx_inuse = true;
    S.gx_split = false;
    S.gen_reset = ctx->gen_pending;                    // the first batch of a fresh generation (hdrf_reset_async)
    ctx->gen_pending = false;
    ctx->gx_nfront++;
    return 0;
}

// Wait for the oldest launched front; its per-peer X1 record counts -> send_counts[G].
extern "C" int hdrf_gx_front_wait(hdrf_ctx *ctx, int64_t *send_counts)
{
    HDRF_LOCK(ctx);
    if (!ctx) return HDRF_E_INVAL;
    if (ctx->gx_nfront <= ctx->gx_nfwait) return set_err(ctx, HDRF_E_INVAL, "hdrf_gx_front_wait: no front pending");
    if (!send_counts) return set_err(ctx, HDRF_E_INVAL, "null counts");
    const int si = (int)(ctx->gx_nfwait % (uint64_t)ctx->gx_depth);
    Slot &S = ctx->sl[si];
    HIPCK(hipEventSynchronize(S.front_done));
    ctx->gx_nfwait++;
    const int herr = S.h_gx->front_err;
    if (herr) {
        HIPCK(hipMemsetAsync(S.d_err, 0, sizeof(int), ctx->stX));
        HIPCK(hipStreamSynchronize(ctx->stX));
        return device_error(ctx, herr);
    }
    S.gx_c1.assign(ctx->G, 0);
    for (int d = 0; d < ctx->G; d++) send_counts[d] = S.gx_c1[(size_t)d] = (int64_t)S.h_gx->front_cnt[d];
    return 0;
}

extern "C" int hdrf_gx_front(hdrf_ctx *ctx, int32_t nblocks, const uint8_t *const *dev_data, const uint64_t *len,
                             const uint64_t *readable, const uint64_t *block_ids, uint32_t gbase, uint32_t *x1_send,
                             int64_t *send_counts)
{
    HDRF_LOCK(ctx);
    if (!send_counts) return ctx ? set_err(ctx, HDRF_E_INVAL, "null counts") : HDRF_E_INVAL;
    if (ctx && ctx->gx_nfront != ctx->gx_nfwait)
        return set_err(ctx, HDRF_E_INVAL, "hdrf_gx_front: launched fronts are pending (hdrf_gx_front_wait)");
    if (int rc = hdrf_gx_front_launch(ctx, nblocks, dev_data, len, readable, block_ids, gbase, x1_send)) return rc;
    return hdrf_gx_front_wait(ctx, send_counts);
}

static Slot &gx_back_slot(hdrf_ctx *ctx) { return ctx->sl[ctx->gx_nback % (uint64_t)ctx->gx_depth]; }
static int gx_back_si(hdrf_ctx *ctx) { return (int)(ctx->gx_nback % (uint64_t)ctx->gx_depth); }

extern "C" int hdrf_gx_owner(hdrf_ctx *ctx, const uint32_t *x1_recv, const int64_t *recv_counts, uint32_t *x2_send)
{
    HDRF_LOCK(ctx);
    if (int rc = gx_check(ctx, 0)) return rc;
    Slot &S = gx_back_slot(ctx);
    if (!x1_recv || !recv_counts || !x2_send) return set_err(ctx, HDRF_E_INVAL, "null exchange buffer");
    for (int s = 0; s < ctx->G; s++)
        if (recv_counts[s] < 0 || recv_counts[s] > ctx->gx_cap) return set_err(ctx, HDRF_E_INVAL, "bad receive count");
    hipStream_t st = ctx->stB;
    const uint64_t seq = ctx->gx_nback;
    if (S.gen_reset) {
        // a fresh generation (hdrf_reset_async): the next epoch of the partition's tag words (the table
        // cleared when it wraps), batches from this one on are this generation's, and the node's
        // allocator re-seeded — on stream B after every older batch's owner..commit phases, and after
        // the last arena copy on B2 (the new generation reuses the slot rings from their start)
        hipEvent_t b2;                                 // everything on B2 so far: older batches' copies
        HIPCK(hipEventCreateWithFlags(&b2, hipEventDisableTiming));
        HIPCK(hipEventRecord(b2, ctx->stB2));
        HIPCK(hipStreamWaitEvent(st, b2, 0));
        HIPCK(hipEventDestroy(b2));
        const bool clear = ctx->epoch >= 255;
        ctx->epoch = clear ? 1 : ctx->epoch + 1;
        ctx->bfirst = S.gx_batch;
        HIPCK(launch_index_clear(ctx->d_tab, clear ? ctx->cfg.index_log2 : -1, ctx->d_alloc, initial_alloc(ctx), st, 0u));
        ctx->h_alloc = initial_alloc(ctx);            // (hdrf_gx_alloc_scan, host form, starts from it)
    }
    gx_mark(ctx, seq, kG0, st);
    std::memcpy(S.h_gx->up_r1, recv_counts, sizeof(int64_t) * ctx->G);
    HIPCK(hipMemcpyAsync(ctx->d_gx_rcounts, S.h_gx->up_r1, sizeof(int64_t) * ctx->G, hipMemcpyHostToDevice, st));
    HIPCK(hipMemsetAsync(ctx->d_gx_x3exp, 0, sizeof(unsigned long long) * ctx->G, st));
    HIPCK(launch_gx_owner(ctx->cfg.hasher, x1_recv, ctx->d_gx_rcounts, max_count(recv_counts, ctx->G), ctx->gx_cap,
                          ctx->G, ctx->d_tab, ctx->cfg.index_log2, S.gx_batch, ctx->bfirst, tag_mask(ctx), ctx->d_oslot,
                          ctx->d_oflags, S.d_coll, S.d_ncoll, ctx->coll_cap, x2_send, ctx->d_gx_x3exp, S.d_err, st));
    gx_mark(ctx, seq, kG1, st);
    // no host round trip: a device error (S.d_err) is read back with the batch by hdrf_gx_place, and
    // the X2 exchange may be enqueued on stream B right behind this kernel (hdrf_gx_stream)
    ctx->gx_bphase = 1;
    return 0;
}

extern "C" int hdrf_gx_stream(hdrf_ctx *ctx, void **stream)
{
    HDRF_LOCK(ctx);
    if (!ctx || !stream) return HDRF_E_INVAL;
    *stream = (void *)ctx->stB;
    return 0;
}

extern "C" int hdrf_gx_decide(hdrf_ctx *ctx, const uint32_t *x2_recv)
{
    HDRF_LOCK(ctx);
    if (int rc = gx_check(ctx, 1)) return rc;
    const int si = gx_back_si(ctx);
    Slot &S = ctx->sl[si];
    if (!x2_recv) return set_err(ctx, HDRF_E_INVAL, "null exchange buffer");
    hipStream_t st = ctx->stB;
    const uint64_t seq = ctx->gx_nback;
    const int nb = S.nblocks;
    gx_mark(ctx, seq, kG2, st);
    HIPCK(launch_gx_decide(S.d_bst, nb, ctx->cap_blk, ctx->ntiles, S.d_off, ctx->d_scratch[si], S.d_slot, x2_recv,
                           S.d_flags, S.d_tilesum, st));
    // the X3 records the owners' answers call for (checked against place_kernel's own counts)
    HIPCK(launch_gx_x3want(x2_recv, ctx->d_gxe[si], max_count(S.gx_c1.data(), ctx->G), ctx->gx_cap, ctx->G,
                           ctx->d_x3want, st));
    gx_mark(ctx, seq, kG3, st);
    const StoreParams P = store_params(ctx, nb);
    HIPCK(launch_store_scan(P, S.d_bst, S.d_off, S.d_flags, S.d_tilesum, S.d_tilepre, S.d_store,
                            S.d_pre, st));
    gx_mark(ctx, seq, kG4, st);
    ctx->gx_x2 = x2_recv;
    ctx->gx_bphase = 2;
    return 0;
}

extern "C" int hdrf_gx_flush(hdrf_ctx *ctx, const uint8_t *alloc_in, uint8_t *alloc_out)
{
    HDRF_LOCK(ctx);
    if (int rc = gx_check(ctx, 2)) return rc;
    Slot &S = gx_back_slot(ctx);
    hipStream_t st = ctx->stB;
    if (alloc_in) {
        ctx->gx_dscan = 0;                             // a host-given allocator replaces the device scan's
        std::memcpy(&ctx->gx_ain, alloc_in, sizeof(AllocState));
        S.h_gx->st[0] = ctx->gx_ain;
        HIPCK(hipMemcpyAsync(ctx->d_alloc, &S.h_gx->st[0], sizeof(AllocState), hipMemcpyHostToDevice, st));
    } else if (!ctx->gx_dscan) {
        HIPCK(hipMemcpyAsync(&S.h_gx->st[0], ctx->d_alloc, sizeof(AllocState), hipMemcpyDeviceToHost, st));
    }
    HIPCK(hipMemsetAsync(S.d_nclosed, 0, sizeof(uint32_t), st));
    const StoreParams P = store_params(ctx, S.nblocks);
    HIPCK(launch_store_flush(P, S.d_bst, S.d_store, S.d_pre, ctx->d_alloc, S.d_rstate, S.d_ev,
                             S.d_closed, S.d_nclosed, S.d_err, st));
    gx_mark(ctx, ctx->gx_nback, kG9, st);
    if (!alloc_out && (ctx->gx_scanned || ctx->gx_dscan)) {   // the scan knows the result: no host round trip
        if (ctx->gx_scanned) ctx->gx_aout = ctx->gx_expect;
        ctx->gx_bphase = 3;
        return 0;
    }
    AllocState a{};
    HIPCK(hipMemcpyAsync(&S.h_gx->st[3], ctx->d_alloc, sizeof a, hipMemcpyDeviceToHost, st));
    if (ctx->gx_dscan) HIPCK(hipMemcpyAsync(S.h_gx->st, ctx->d_gxst, 2 * sizeof a, hipMemcpyDeviceToHost, st));
    HIPCK(hipStreamSynchronize(st));
    a = S.h_gx->st[3];
    if (!alloc_in) ctx->gx_ain = S.h_gx->st[0];
    ctx->gx_aout = a;
    if (ctx->gx_scanned && std::memcmp(&a, &ctx->gx_expect, sizeof a) != 0)
        return set_err(ctx, HDRF_E_DEVICE, "allocator scan disagrees with the flush walk");
    if (ctx->gx_dscan && std::memcmp(&a, &S.h_gx->st[1], sizeof a) != 0)
        return set_err(ctx, HDRF_E_DEVICE, "device allocator scan disagrees with the flush walk");
    if (alloc_out) {
        std::memset(alloc_out, 0, HDRF_ALLOC_STATE_BYTES);
        std::memcpy(alloc_out, &a, sizeof a);
    }
    ctx->gx_bphase = 3;
    return 0;
}

// ---- allocator scan: every rank's flush walk as a function of the incoming allocator ------
// (store.hip fn_info / fn_chain).  Host descriptor, int64 words: n_thread, then per range t
// {any, S, base_last, S_last, m, m x (v, final container start, closes after the first)}.

// fn_info / fn_chain into the context's scratch (the candidate rows per range); returns the scratch
static int gx_flush_rows(hdrf_ctx *ctx, Slot &S, int *err, uint8_t **F_out)
{
    hipStream_t st = ctx->stB;
    const StoreParams P = store_params(ctx, S.nblocks);
    const int64_t kcap = (int64_t)ctx->max_batch * ctx->cap_blk + 1;
    const uint64_t o_fr = 64 * 4 * sizeof(FnBlock), o_k = o_fr + 256, o_out = o_k + 256;
    if (int rc = grow(ctx, &ctx->d_fn, &ctx->fn_cap, o_out + (uint64_t)P.n_thread * kcap * 24)) return rc;
    uint8_t *F = ctx->d_fn;
    HIPCK(hipMemsetAsync(F + o_k, 0, 64, st));
    HIPCK(launch_flush_fn(P, S.d_bst, S.d_store, S.d_pre, (FnBlock *)F, (FnRange *)(F + o_fr), (uint64_t *)(F + o_out),
                          kcap, (unsigned long long *)(F + o_k), err, st));
    *F_out = F;
    return 0;
}

extern "C" int64_t hdrf_gx_flush_fn(hdrf_ctx *ctx, int64_t *desc, int64_t cap)
{
    HDRF_LOCK(ctx);
    if (int rc = gx_check(ctx, 2)) return rc;
    Slot &S = gx_back_slot(ctx);
    hipStream_t st = ctx->stB;
    const int nt = ctx->cfg.n_thread;
    const int64_t kcap = (int64_t)ctx->max_batch * ctx->cap_blk + 1;
    const uint64_t o_fr = 64 * 4 * sizeof(FnBlock), o_k = o_fr + 256, o_out = o_k + 256;
    uint8_t *F = nullptr;
    // (the function's own error word after the rows; read back with the rows' counts)
    if (int rc = grow(ctx, &ctx->d_fn, &ctx->fn_cap, o_out + (uint64_t)nt * kcap * 24 + 64)) return rc;
    int *d_err = (int *)(ctx->d_fn + o_out + (uint64_t)nt * kcap * 24);
    HIPCK(hipMemsetAsync(d_err, 0, sizeof(int), st));
    if (int rc = gx_flush_rows(ctx, S, d_err, &F)) return rc;
    FnRange fr[4];
    unsigned long long K[4];
    int herr = 0;
    HIPCK(hipMemcpyAsync(fr, F + o_fr, sizeof(FnRange) * nt, hipMemcpyDeviceToHost, st));
    HIPCK(hipMemcpyAsync(K, F + o_k, 8 * nt, hipMemcpyDeviceToHost, st));
    HIPCK(hipMemcpyAsync(&herr, d_err, 4, hipMemcpyDeviceToHost, st));
    HIPCK(hipStreamSynchronize(st));
    if (herr) return set_err(ctx, HDRF_E_DEVICE, "flush function: candidate table overflow or runaway chain");
    std::vector<uint64_t> rows[4];
    for (int t = 0; t < nt; t++) {
        rows[t].resize(3 * K[t]);
        if (K[t]) HIPCK(hipMemcpyAsync(rows[t].data(), F + o_out + (uint64_t)t * kcap * 24, 24 * K[t], hipMemcpyDeviceToHost, st));
    }
    HIPCK(hipStreamSynchronize(st));
    std::vector<int64_t> d{nt};
    for (int t = 0; t < nt; t++) {
        const size_t h = d.size();
        d.insert(d.end(), {(int64_t)fr[t].any, (int64_t)fr[t].S, (int64_t)fr[t].base_last, (int64_t)fr[t].S_last, 0});
        int64_t m = 0;
        for (uint64_t i = 0; i < K[t]; i++) {
            const uint64_t *r = &rows[t][3 * i];
            if (r[2] >> 63) continue;                      // repeats the previous prefix
            d.insert(d.end(), {(int64_t)r[0], (int64_t)r[1], (int64_t)r[2]});
            m++;
        }
        if (fr[t].any && (m == 0 || d[h + 5] != 0)) return set_err(ctx, HDRF_E_DEVICE, "flush function: no start candidate");
        d[h + 4] = m;
    }
    if (!desc || cap < (int64_t)d.size()) {
        if (cap >= 0) set_err(ctx, HDRF_E_CAPACITY, "flush descriptor needs " + std::to_string(d.size()) + " words");
        return -(int64_t)d.size() - 1000;           // callers size with the returned -(n + 1000)
    }
    std::copy(d.begin(), d.end(), desc);
    return (int64_t)d.size();
}

// The same function packed on the device into a fixed-size descriptor of hdrf_gx_layout.fn_bytes
// (store.hip fn_pack_kernel), enqueued on the back stream: the ranks all-gather the descriptors
// there and hdrf_gx_alloc_scan_dev composes them, with no host round trip.
extern "C" int hdrf_gx_flush_fn_dev(hdrf_ctx *ctx, void *dev_desc)
{
    HDRF_LOCK(ctx);
    if (int rc = gx_check(ctx, 2)) return rc;
    if (!dev_desc) return set_err(ctx, HDRF_E_INVAL, "null descriptor buffer");
    Slot &S = gx_back_slot(ctx);
    hipStream_t st = ctx->stB;
    const int nt = ctx->cfg.n_thread;
    const int64_t kcap = (int64_t)ctx->max_batch * ctx->cap_blk + 1;
    const uint64_t o_fr = 64 * 4 * sizeof(FnBlock), o_k = o_fr + 256, o_out = o_k + 256;
    gx_mark(ctx, ctx->gx_nback, kG5, st);
    uint8_t *F = nullptr;
    if (int rc = gx_flush_rows(ctx, S, S.d_err, &F)) return rc;
    HIPCK(launch_fn_pack(nt, (const FnRange *)(F + o_fr), (const uint64_t *)(F + o_out), kcap,
                         (const unsigned long long *)(F + o_k), ctx->fn_mcap, dev_desc, S.d_err, st));
    gx_mark(ctx, ctx->gx_nback, kG6, st);
    return 0;
}

// one rank's flush function applied to the allocator A (the walk of store.hip flush_kernel)
static bool gx_apply_fn(const hdrf_ctx *ctx, const int64_t *d, int64_t len, AllocState &A)
{
    if (len < 1) return false;
    const int nt = (int)d[0];
    if (nt != ctx->cfg.n_thread) return false;
    const int64_t cmax = (int64_t)ctx->cfg.container_max;
    const uint32_t per = (uint32_t)(ctx->cfg.arena_slots / 4);
    int64_t p = 1;
    for (int t = 0; t < nt; t++) {
        if (p + 5 > len) return false;
        const int64_t any = d[p], S = d[p + 1], bl = d[p + 2], Sl = d[p + 3], m = d[p + 4];
        const int64_t *v = d + p + 5;
        p += 5 + 3 * m;
        if (m < 0 || p > len) return false;
        if (!any) continue;
        const int64_t x = A.exists[t] ? (int64_t)A.cur[t] : 0;
        int64_t cs = -x, n = 0;
        if (x + S > cmax) {
            const int64_t thr = cmax - x;              // first close after the last prefix <= thr
            int64_t lo = 0, hi = m;                    // largest v <= thr (v_0 = 0 <= thr)
            while (hi - lo > 1) {
                const int64_t mid = (lo + hi) / 2;
                if (v[3 * mid] <= thr) lo = mid; else hi = mid;
            }
            cs = v[3 * lo + 1];
            n = 1 + v[3 * lo + 2];
        }
        const uint32_t base = (uint32_t)t * per;
        A.id[t] += (uint32_t)n;
        A.slot[t] = base + (uint32_t)(((int64_t)(A.slot[t] - base) + n) % per);
        A.cur[t] = (uint32_t)(S - cs);
        A.exists[t] = 1;
        A.pos[t] = (uint32_t)(Sl - std::max<int64_t>(cs - bl, 0));
    }
    return p == len;
}

// The node's allocator for this batch from every rank's flush function (rank order): the state
// this rank's flush walk starts from (the exclusive scan) and the state after the last rank.
extern "C" int hdrf_gx_alloc_scan(hdrf_ctx *ctx, const int64_t *descs, const int64_t *lens, uint8_t *alloc_in,
                                  uint8_t *alloc_final)
{
    HDRF_LOCK(ctx);
    if (int rc = gx_check(ctx, 2)) return rc;
    if (!descs || !lens || !alloc_in || !alloc_final) return set_err(ctx, HDRF_E_INVAL, "null scan argument");
    AllocState A = ctx->h_alloc;
    int64_t off = 0;
    for (int r = 0; r < ctx->G; r++) {
        if (r == ctx->cfg.rank) {
            std::memset(alloc_in, 0, HDRF_ALLOC_STATE_BYTES);
            std::memcpy(alloc_in, &A, sizeof A);
        }
        if (lens[r] < 1 || !gx_apply_fn(ctx, descs + off, lens[r], A))
            return set_err(ctx, HDRF_E_INVAL, "malformed flush descriptor of rank " + std::to_string(r));
        if (r == ctx->cfg.rank) ctx->gx_expect = A;
        off += lens[r];
    }
    std::memset(alloc_final, 0, HDRF_ALLOC_STATE_BYTES);
    std::memcpy(alloc_final, &A, sizeof A);
    ctx->gx_scanned = 1;
    return 0;
}

// The same composition on the device over the all-gathered descriptors (G x fn_bytes, rank order):
// the node's allocator after the previous batch (on the device already) -> this rank's incoming
// state for hdrf_gx_flush(ctx, NULL, NULL), its predicted result (checked by hdrf_gx_place) and the
// node's state after the batch (installed by hdrf_gx_place).  Enqueued on the back stream.
extern "C" int hdrf_gx_alloc_scan_dev(hdrf_ctx *ctx, const void *dev_descs)
{
    HDRF_LOCK(ctx);
    if (int rc = gx_check(ctx, 2)) return rc;
    if (!dev_descs) return set_err(ctx, HDRF_E_INVAL, "null descriptors");
    Slot &S = gx_back_slot(ctx);
    hipStream_t st = ctx->stB;
    gx_mark(ctx, ctx->gx_nback, kG7, st);
    HIPCK(launch_gx_scan(dev_descs, ctx->fn_bytes, ctx->G, ctx->cfg.rank, ctx->cfg.n_thread,
                         (uint32_t)(ctx->cfg.arena_slots / 4), ctx->cfg.container_max, ctx->d_alloc, ctx->d_gxst,
                         S.d_err, st));
    gx_mark(ctx, ctx->gx_nback, kG8, st);
    ctx->gx_dscan = 1;
    ctx->gx_scanned = 0;
    return 0;
}

// Placement of the back batch: on stream B the per-chunk container positions, the X3 location
// records and the read-back the host needs (hdrf_gx_place_wait); the arena copy of the new chunks
// runs on stream B2 (compressor 2 keeps it on B: its LZ4 pass reads the containers there).
extern "C" int hdrf_gx_place_launch(hdrf_ctx *ctx, const uint8_t *alloc_final, uint32_t *x3_send)
{
    HDRF_LOCK(ctx);
    if (int rc = gx_check(ctx, 3)) return rc;
    if (ctx->gx_place_pending) return set_err(ctx, HDRF_E_INVAL, "hdrf_gx_place_launch: a placement is pending");
    const int si = gx_back_si(ctx);
    Slot &S = ctx->sl[si];
    if (!x3_send) return set_err(ctx, HDRF_E_INVAL, "null exchange buffer");
    if (!alloc_final && !ctx->gx_dscan)
        return set_err(ctx, HDRF_E_INVAL, "hdrf_gx_place: the node's allocator (alloc_final) is needed without the device scan");
    hipStream_t st = ctx->stB;
    const uint64_t seq = ctx->gx_nback;
    const int nb = S.nblocks;
    const StoreParams P = store_params(ctx, nb);
    const bool split = ctx->cfg.compressor != 2;
    GxPlace gx;
    gx.x2 = ctx->gx_x2; gx.x3 = x3_send; gx.cap = ctx->gx_cap; gx.counts = ctx->d_gx_counts; gx.G = ctx->G;
    gx.part = split ? 1 : 0;
    gx_mark(ctx, seq, kG10, st);
    HIPCK(launch_store_place(P, S.d_blocks, S.d_bst, S.d_off, S.d_flags, S.d_pre, S.d_rstate, S.d_ev, S.d_slot,
                             ctx->d_scratch[si], ctx->d_arena, S.d_pcid, S.d_ppos, gx, st));
    // the flush walk's result (checked against the scan), then the node's allocator after the batch
    // (the next batch and the "blockID" view start from it)
    HIPCK(hipMemcpyAsync(ctx->d_gxst + 3, ctx->d_alloc, sizeof(AllocState), hipMemcpyDeviceToDevice, st));
    if (alloc_final) {
        std::memcpy(&S.h_gx->st[2], alloc_final, sizeof(AllocState));
        HIPCK(hipMemcpyAsync(ctx->d_alloc, &S.h_gx->st[2], sizeof(AllocState), hipMemcpyHostToDevice, st));
    } else {
        HIPCK(hipMemcpyAsync(ctx->d_alloc, ctx->d_gxst + 2, sizeof(AllocState), hipMemcpyDeviceToDevice, st));
    }
    GxHost *h = S.h_gx;
    HIPCK(hipMemcpyAsync(h->c3, ctx->d_gx_counts, sizeof(unsigned long long) * ctx->G, hipMemcpyDeviceToHost, st));
    HIPCK(hipMemcpyAsync(h->x3e, ctx->d_gx_x3exp, sizeof(unsigned long long) * ctx->G, hipMemcpyDeviceToHost, st));
    HIPCK(hipMemcpyAsync(h->x3want, ctx->d_x3want, sizeof(unsigned long long) * ctx->G, hipMemcpyDeviceToHost, st));
    HIPCK(hipMemcpyAsync(&h->commit_err, ctx->d_gx_err, sizeof(int), hipMemcpyDeviceToHost, st));
    if (ctx->gx_dscan) HIPCK(hipMemcpyAsync(h->st, ctx->d_gxst, 2 * sizeof(AllocState), hipMemcpyDeviceToHost, st));
    HIPCK(hipMemcpyAsync(&h->st[3], ctx->d_gxst + 3, sizeof(AllocState), hipMemcpyDeviceToHost, st));
    HIPCK(hipMemcpyAsync(S.h_bst, S.d_bst, sizeof(BlockState) * nb, hipMemcpyDeviceToHost, st));
    HIPCK(hipMemcpyAsync(S.h_store, S.d_store, sizeof(uint64_t) * nb, hipMemcpyDeviceToHost, st));
    HIPCK(hipMemcpyAsync(S.h_alloc, ctx->d_alloc, sizeof(AllocState), hipMemcpyDeviceToHost, st));
    HIPCK(hipMemcpyAsync(S.h_err, S.d_err, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCK(hipMemcpyAsync(S.h_nclosed, S.d_nclosed, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIPCK(hipMemcpyAsync(S.h_closed, S.d_closed, sizeof(ClosedRec) * ctx->closed_cap, hipMemcpyDeviceToHost, st));
    gx_mark(ctx, seq, kG11, st);
    HIPCK(hipEventRecord(S.gx_meta, st));
    if (split) {                                        // the arena copy beside the next batch's owner phases
        hipStream_t B2 = ctx->stB2;
        HIPCK(hipStreamWaitEvent(B2, S.gx_meta, 0));
        gx.part = 2;
        gx_mark(ctx, seq, kP0, B2);
        HIPCK(launch_store_place(P, S.d_blocks, S.d_bst, S.d_off, S.d_flags, S.d_pre, S.d_rstate, S.d_ev, S.d_slot,
                                 ctx->d_scratch[si], ctx->d_arena, S.d_pcid, S.d_ppos, gx, B2));
        gx_mark(ctx, seq, kP1, B2);
        HIPCK(hipEventRecord(S.placed, B2));
        S.gx_split = true;
    }
    ctx->gx_place_pending = true;
    return 0;
}

// Wait for the placement's read-back: this rank's X3 send counts (send_counts[G]), the checks of
// the allocator scan and of the X3 counts, and the host bookkeeping of the batch.
extern "C" int hdrf_gx_place_wait(hdrf_ctx *ctx, int64_t *send_counts)
{
    HDRF_LOCK(ctx);
    if (int rc = gx_check(ctx, 3)) return rc;
    if (!ctx->gx_place_pending) return set_err(ctx, HDRF_E_INVAL, "hdrf_gx_place_wait: no placement launched");
    if (!send_counts) return set_err(ctx, HDRF_E_INVAL, "null counts");
    const int si = gx_back_si(ctx);
    Slot &S = ctx->sl[si];
    GxHost *h = S.h_gx;
    HIPCK(hipEventSynchronize(S.gx_meta));
    ctx->gx_place_pending = false;
    if (h->commit_err) {                               // an earlier batch's commit (not waited for)
        HIPCK(hipMemsetAsync(ctx->d_gx_err, 0, sizeof(int), ctx->stB));
        HIPCK(hipStreamSynchronize(ctx->stB));
        const int e = h->commit_err;
        h->commit_err = 0;
        return device_error(ctx, e);
    }
    if (ctx->gx_dscan) {
        ctx->gx_ain = h->st[0];
        ctx->gx_aout = h->st[3];
        if (!*S.h_err && std::memcmp(&h->st[3], &h->st[1], sizeof(AllocState)) != 0)
            return set_err(ctx, HDRF_E_DEVICE, "device allocator scan disagrees with this rank's flush walk");
    } else if (ctx->gx_scanned) {
        if (std::memcmp(&h->st[3], &ctx->gx_expect, sizeof(AllocState)) != 0)
            return set_err(ctx, HDRF_E_DEVICE, "allocator scan disagrees with this rank's flush walk");
    }
    ctx->gx_scanned = 0;
    ctx->gx_dscan = 0;
    if (S.gen_reset && !*S.h_err) {                    // the fresh generation's host side (hdrf_reset_async)
        reset_host(ctx);
        ctx->h_alloc = initial_alloc(ctx);
        S.gen_reset = false;
    }
    // (checked before any host bookkeeping: a failed placement leaves the host state untouched; a
    // device error is complete_slot's to report)
    for (int d = 0; d < ctx->G && !*S.h_err; d++)
        if (h->c3[d] != h->x3want[d])
            return set_err(ctx, HDRF_E_DEVICE, "X3 send count to rank " + std::to_string(d) + " (" +
                                                   std::to_string(h->c3[d]) + ") disagrees with its X2 answers (" +
                                                   std::to_string(h->x3want[d]) + ")");
    // the open containers this rank's flush walk started and ended in hold its placed chunks even
    // when another rank closes them (the node read, hdrf_gx_read_fill, gathers from them)
    for (const AllocState *a : {&ctx->gx_ain, &ctx->gx_aout})
        for (int t = 0; t < ctx->cfg.n_thread; t++)
            if (a->exists[t] && !ctx->containers.count(a->id[t])) note_container(ctx, a->id[t], a->slot[t], a->cur[t], 0);
    S.gx_compressed = false;
    if (int rc = complete_slot(ctx, si, false)) return rc;
    for (int d = 0; d < ctx->G; d++) send_counts[d] = (int64_t)h->c3[d];
    ctx->gx_x3recv.assign(h->x3e, h->x3e + ctx->G);
    ctx->gx_bphase = 4;
    gx_collect(ctx, false, ctx->gx_nback);
    return 0;
}

extern "C" int hdrf_gx_place(hdrf_ctx *ctx, const uint8_t *alloc_final, uint32_t *x3_send, int64_t *send_counts)
{
    HDRF_LOCK(ctx);
    if (!send_counts) return ctx ? set_err(ctx, HDRF_E_INVAL, "null exchange buffer") : HDRF_E_INVAL;
    if (int rc = hdrf_gx_place_launch(ctx, alloc_final, x3_send)) return rc;
    return hdrf_gx_place_wait(ctx, send_counts);
}

// The X3 receive counts this owner's decisions imply (valid from hdrf_gx_place to hdrf_gx_commit):
// the X3 exchange needs no count exchange of its own.
extern "C" int hdrf_gx_x3_counts(hdrf_ctx *ctx, int64_t *recv_counts)
{
    HDRF_LOCK(ctx);
    if (int rc = gx_check(ctx, 4)) return rc;
    if (!recv_counts) return set_err(ctx, HDRF_E_INVAL, "null counts");
    for (int s = 0; s < ctx->G; s++) recv_counts[s] = ctx->gx_x3recv[(size_t)s];
    return 0;
}

// ---- node-global compressor 2 (DN/DataDeduplicator.java:748-797: a closing container is rewritten
// as one Lz4Codec file).  A node-global container's bytes lie on the ranks that placed into it (rank
// r continues the container rank r - 1 left open, in the same arena slot index), so the rank whose
// flush walk closes a container first gathers the head pieces the earlier ranks hold
// (hdrf_gx_piece, planned on the host from every rank's hdrf_gx_alloc_io), then compresses the
// containers it closed (hdrf_gx_compress), all between hdrf_gx_place and hdrf_gx_commit.
extern "C" int hdrf_gx_alloc_io(hdrf_ctx *ctx, uint8_t *alloc_in, uint8_t *alloc_out)
{
    HDRF_LOCK(ctx);
    if (!ctx || ctx->G < 2 || !alloc_in || !alloc_out) return ctx ? set_err(ctx, HDRF_E_INVAL, "bad arguments") : HDRF_E_INVAL;
    if (ctx->gx_bphase != 4 && !(ctx->gx_bphase == 3 && !ctx->gx_place_pending && !ctx->gx_dscan))
        return set_err(ctx, HDRF_E_INVAL, "hdrf_gx_alloc_io after hdrf_gx_flush (or hdrf_gx_place with the device scan)");
    std::memset(alloc_in, 0, HDRF_ALLOC_STATE_BYTES);
    std::memcpy(alloc_in, &ctx->gx_ain, sizeof(AllocState));
    std::memset(alloc_out, 0, HDRF_ALLOC_STATE_BYTES);
    std::memcpy(alloc_out, &ctx->gx_aout, sizeof(AllocState));
    return 0;
}

extern "C" int hdrf_gx_piece(hdrf_ctx *ctx, uint32_t id, uint64_t off, uint64_t n, void *dev, int32_t write)
{
    HDRF_LOCK(ctx);
    if (!ctx || ctx->G < 2 || (n && !dev)) return ctx ? set_err(ctx, HDRF_E_INVAL, "bad arguments") : HDRF_E_INVAL;
    if (write && ctx->cfg.compressor != 2)
        return set_err(ctx, HDRF_E_INVAL, "hdrf_gx_piece: writes are the compressor-2 head-piece gather only");
    auto it = ctx->containers.find(id);
    if (it == ctx->containers.end()) return set_err(ctx, HDRF_E_NOTFOUND, "container not resident on this rank");
    if (off > ctx->cfg.container_max || n > ctx->cfg.container_max - off) return set_err(ctx, HDRF_E_INVAL, "piece outside the container");
    uint8_t *p = ctx->d_arena + (size_t)it->second.slot * ctx->cfg.container_max + off;
    if (n) {
        // (an arena copy of this rank's place on stream B2 must have landed before a read)
        for (auto &S : ctx->sl)
            if (S.gx_inuse && S.gx_split) HIPCK(hipStreamWaitEvent(ctx->stB, S.placed, 0));
        HIPCK(hipMemcpyAsync(write ? (void *)p : dev, write ? (const void *)dev : (const void *)p, n, hipMemcpyDeviceToDevice,
                             ctx->stB));
        // a read hands the bytes to the caller (who ships them to the closer): complete on return; a
        // write is ordered before hdrf_gx_compress on the same stream, which synchronises
        if (!write) HIPCK(hipStreamSynchronize(ctx->stB));
    }
    return 0;
}

extern "C" int hdrf_gx_compress(hdrf_ctx *ctx)
{
    HDRF_LOCK(ctx);
    if (!ctx) return HDRF_E_INVAL;
    // every return path leaves the queued hdrf_gx_piece writes complete (their source buffers may be
    // released by the caller as soon as this returns)
    if (int rc = gx_check(ctx, 4)) {
        if (ctx->stB) (void)hipStreamSynchronize(ctx->stB);
        return rc;
    }
    const hdrf_cfg &c = ctx->cfg;
    if (c.compressor != 2) {
        HIPCK(hipStreamSynchronize(ctx->stB));
        return 0;
    }
    Slot &S = gx_back_slot(ctx);
    const uint32_t nclosed = *S.h_nclosed;
    if (!nclosed || S.gx_compressed) {                  // once per batch: a second call changes nothing
        HIPCK(hipStreamSynchronize(ctx->stB));         // (hdrf_gx_piece writes are complete on return)
        return 0;
    }
    hipStream_t st = ctx->stB;
    HIPCK(launch_lz4(S.d_closed, S.d_nclosed, ctx->closed_cap, c.container_max, ctx->d_arena, ctx->d_carena, ctx->cslot,
                     S.d_segclen, S.d_filelen, S.d_lzwork, st));
    HIPCK(hipMemcpyAsync(S.h_filelen, S.d_filelen, sizeof(uint32_t) * nclosed, hipMemcpyDeviceToHost, st));
    HIPCK(hipStreamSynchronize(st));
    for (uint32_t i = 0; i < nclosed; i++) {
        const ClosedRec &r = S.h_closed[i];
        auto it = ctx->containers.find(r.id);
        if (it == ctx->containers.end()) return set_err(ctx, HDRF_E_DEVICE, "closed container missing");
        it->second.clen = S.h_filelen[i];
        ctx->stats.closed_file_bytes += (int64_t)S.h_filelen[i] - (int64_t)r.len;
    }
    S.gx_compressed = true;
    return (int)nclosed;
}

// The owners' commit of the X3 locations: enqueued on the back stream and not waited for (an
// error it raises is reported by the next hdrf_gx_place or by hdrf_gx_sync).
extern "C" int hdrf_gx_commit(hdrf_ctx *ctx, const uint32_t *x3_recv, const int64_t *recv_counts)
{
    HDRF_LOCK(ctx);
    if (int rc = gx_check(ctx, 4)) return rc;
    if (!x3_recv || !recv_counts) return set_err(ctx, HDRF_E_INVAL, "null exchange buffer");
    for (int s = 0; s < ctx->G; s++) {
        if (recv_counts[s] < 0 || recv_counts[s] > ctx->gx_cap) return set_err(ctx, HDRF_E_INVAL, "bad receive count");
        if (recv_counts[s] != ctx->gx_x3recv[(size_t)s])
            return set_err(ctx, HDRF_E_DEVICE, "X3 receive count from rank " + std::to_string(s) +
                                                   " disagrees with this owner's decisions");
    }
    Slot &S = gx_back_slot(ctx);
    // compressor 2: the containers this rank closed must be Lz4Codec files before the batch commits
    // (container reads of closed containers take their bytes from the compressed arena)
    if (ctx->cfg.compressor == 2 && *S.h_nclosed && !S.gx_compressed)
        return set_err(ctx, HDRF_E_INVAL, "compressor 2: hdrf_gx_compress must run between hdrf_gx_place and hdrf_gx_commit");
    hipStream_t st = ctx->stB;
    const uint64_t seq = ctx->gx_nback;
    std::memcpy(S.h_gx->up_r3, recv_counts, sizeof(int64_t) * ctx->G);
    gx_mark(ctx, seq, kG12, st);
    HIPCK(hipMemcpyAsync(ctx->d_gx_rcounts, S.h_gx->up_r3, sizeof(int64_t) * ctx->G, hipMemcpyHostToDevice, st));
    HIPCK(launch_gx_commit(x3_recv, ctx->d_gx_rcounts, max_count(recv_counts, ctx->G), ctx->gx_cap, ctx->G, ctx->d_tab,
                           ctx->cfg.index_log2, ctx->d_gx_err, st));
    gx_mark(ctx, seq, kG13, st);
    HIPCK(hipEventRecord(S.back_done, st));
    ctx->gx_bphase = 0;
    ctx->gx_nback++;
    return 0;
}

// Complete every node-global batch in flight (all streams) and report an error of the last commits.
static int gx_sync_locked(hdrf_ctx *ctx)
{
    if (int rc = drain(ctx)) return rc;
    int herr = 0;
    HIPCK(hipMemcpy(&herr, ctx->d_gx_err, sizeof(int), hipMemcpyDeviceToHost));
    gx_collect(ctx, true, ctx->gx_nback);
    if (herr) {
        HIPCK(hipMemset(ctx->d_gx_err, 0, sizeof(int)));
        return device_error(ctx, herr);
    }
    return 0;
}

extern "C" int hdrf_gx_sync(hdrf_ctx *ctx)
{
    HDRF_LOCK(ctx);
    if (!ctx) return HDRF_E_INVAL;
    if (ctx->G < 2) return set_err(ctx, HDRF_E_INVAL, "hdrf_gx_* needs cfg.n_ranks > 1");
    return gx_sync_locked(ctx);
}

// ---- node-global read (G > 1): DataConstructor over the node's one index ------------------
// Every rank takes part (include/hdrf.h): the owners locate the digests they own, the locations
// are combined (sum of disjoint rows), and every rank gathers the chunks it placed; the partial
// blocks are disjoint, so their byte sum on the reading rank is the block (hdrf_amd/node.py).
extern "C" int64_t hdrf_gx_read_locate(hdrf_ctx *ctx, const uint8_t *digests, int64_t n, uint32_t *loc)
{
    HDRF_LOCK(ctx);
    if (!ctx) return HDRF_E_INVAL;
    if (ctx->G < 2) return set_err(ctx, HDRF_E_INVAL, "hdrf_gx_read_* needs cfg.n_ranks > 1");
    if (n < 0 || (n && (!digests || !loc))) return set_err(ctx, HDRF_E_INVAL, "bad locate arguments");
    if (n == 0) return 0;
    if (ctx->gx_nfront != ctx->gx_nback) return set_err(ctx, HDRF_E_INVAL, "hdrf_gx_read_locate: a batch is in flight");
    // the last batch's commit (stream B) and arena copy (stream B2) land first; a commit error is reported here
    if (int rc = gx_sync_locked(ctx)) return rc;
    const uint64_t o_loc = (((uint64_t)n * ctx->H) + 255) & ~255ull, o_err = o_loc + (((uint64_t)n * 16 + 255) & ~255ull);
    if (int rc = grow(ctx, &ctx->d_rd, &ctx->rd_cap, o_err + 256)) return rc;
    uint8_t *R = ctx->d_rd;
    hipStream_t st = ctx->st;
    HIPCK(hipMemcpyAsync(R, digests, (size_t)n * ctx->H, hipMemcpyHostToDevice, st));
    HIPCK(hipMemsetAsync(R + o_err, 0, 4, st));
    HIPCK(launch_gx_locate(ctx->cfg.hasher, (const uint32_t *)R, (int)n, ctx->d_tab, ctx->cfg.index_log2, tag_mask(ctx),
                           ctx->G, ctx->cfg.rank, (uint32_t *)(R + o_loc), (int *)(R + o_err), st));
    int herr = 0;
    HIPCK(hipMemcpyAsync(loc, R + o_loc, (size_t)n * 16, hipMemcpyDeviceToHost, st));
    HIPCK(hipMemcpyAsync(&herr, R + o_err, 4, hipMemcpyDeviceToHost, st));
    HIPCK(hipStreamSynchronize(st));
    if (herr) return set_err(ctx, HDRF_E_NOTFOUND, "a recipe digest owned by this rank is not in its index partition");
    int64_t mine = 0;
    for (int64_t k = 0; k < n; k++) mine += loc[4 * k + 3] != 0;
    return mine;
}

extern "C" int64_t hdrf_gx_read_fill(hdrf_ctx *ctx, const uint32_t *loc, int64_t n, uint8_t *dev_out, int64_t cap)
{
    HDRF_LOCK(ctx);
    if (!ctx) return HDRF_E_INVAL;
    if (ctx->G < 2) return set_err(ctx, HDRF_E_INVAL, "hdrf_gx_read_* needs cfg.n_ranks > 1");
    if (n < 0 || (n && !loc)) return set_err(ctx, HDRF_E_INVAL, "bad fill arguments");
    if (ctx->gx_nfront != ctx->gx_nback) return set_err(ctx, HDRF_E_INVAL, "hdrf_gx_read_fill: a batch is in flight");
    if (int rc = gx_sync_locked(ctx)) return rc;
    std::vector<RdChunk> mine;
    std::vector<uint64_t> bases;
    std::map<uint32_t, uint32_t> base_of;               // container id -> index in bases
    uint64_t off = 0, filled = 0;
    for (int64_t k = 0; k < n; k++) {
        const uint32_t *r = loc + 4 * k;
        if (r[3] == 0 || r[2] < r[1]) return set_err(ctx, HDRF_E_INVAL, "location without its placing rank");
        const uint32_t len = r[2] - r[1];
        if ((int)r[3] - 1 == ctx->cfg.rank && len) {
            auto it = ctx->containers.find(r[0]);
            if (it == ctx->containers.end()) return set_err(ctx, HDRF_E_NOTFOUND, "container of a placed chunk is not resident");
            auto b = base_of.find(r[0]);
            if (b == base_of.end()) {
                b = base_of.emplace(r[0], (uint32_t)bases.size()).first;
                bases.push_back((uint64_t)(uintptr_t)(ctx->d_arena + (size_t)it->second.slot * ctx->cfg.container_max));
            }
            if ((uint64_t)r[2] > ctx->cfg.container_max) return set_err(ctx, HDRF_E_DEVICE, "chunk beyond its container");
            mine.push_back(RdChunk{b->second, r[1], len, (uint32_t)off});
            filled += len;
        }
        off += len;
    }
    if ((int64_t)off > cap || (off && !dev_out)) return set_err(ctx, HDRF_E_CAPACITY, "output capacity");
    if (!mine.empty()) {
        const uint64_t o_b = ((mine.size() * sizeof(RdChunk)) + 255) & ~255ull;
        if (int rc = grow(ctx, &ctx->d_rd, &ctx->rd_cap, o_b + bases.size() * 8 + 256)) return rc;
        uint8_t *R = ctx->d_rd;
        hipStream_t st = ctx->st;
        HIPCK(hipMemcpyAsync(R, mine.data(), mine.size() * sizeof(RdChunk), hipMemcpyHostToDevice, st));
        HIPCK(hipMemcpyAsync(R + o_b, bases.data(), bases.size() * 8, hipMemcpyHostToDevice, st));
        HIPCK(launch_rd_gather((const RdChunk *)R, (int)mine.size(), (const uint64_t *)(R + o_b), dev_out, st));
        HIPCK(hipStreamSynchronize(st));
    }
    return (int64_t)filled;
}
