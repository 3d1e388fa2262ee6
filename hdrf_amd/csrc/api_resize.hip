// api_resize.hip — libhdrf C-ABI: the size of the fingerprint table, online (kernel in resize.hip, the
// checks and the byte counts in resize_plan.hpp).
//
// hdrf_index_info_get is a view: it drains the pipeline and writes nothing but the grown scratch (d_rd).
// hdrf_index_resize drains the pipeline, grows d_rd and, when every check has passed, writes d_tab,
// cfg.index_log2 and probe_stale — nothing else.  The old table is only read until then, so there is no
// `lost` path: every failure frees the new table and leaves the context as it was.
#include "ctx.hpp"
#include "resize_plan.hpp"

static_assert(sizeof(hdrf_index_info) == 32, "hdrf_index_info: ctypes mirror IndexInfo in hdrf_amd/lib.py");
static_assert(kIndexMinLog2 == 10 && kIndexMaxLog2 == 31, "hdrf_open's bounds on cfg.index_log2 (api.hip)");

// Enqueue the count of the live entries of a table: the count-only mode of the GC sweep, into the
// GcCounters at scratch offset `off` (cleared here).
static hipError_t enqueue_count(hdrf_ctx *ctx, const IndexEntry *tab, int log2cap, uint64_t off)
{
    hipError_t e = hipMemsetAsync(ctx->d_rd + off, 0, sizeof(GcCounters), ctx->st);
    if (e == hipSuccess)
        e = launch_gc_sweep(ctx->cfg.hasher, tab, log2cap, tag_mask(ctx), nullptr, nullptr, 0, nullptr, nullptr, nullptr,
                            nullptr, 0, nullptr, (GcCounters *)(ctx->d_rd + off), 4 * ctx->n_cu, ctx->st);
    return e;
}

// The live entries of the context's table (the caller drained).
static int count_live(hdrf_ctx *ctx, uint64_t *entries, StageTimer *tm)
{
    if (int rc = grow(ctx, &ctx->d_rd, &ctx->rd_cap, kResizeScratch)) return rc == HDRF_E_HIP ? HDRF_E_NOMEM : rc;
    GcCounters c{};
    if (tm) tm->mark(0, ctx->st);
    HIPCK(enqueue_count(ctx, ctx->d_tab, ctx->cfg.index_log2, kResizeCntOld));
    if (tm) tm->mark(1, ctx->st);
    HIPCK(hipMemcpyAsync(&c, ctx->d_rd + kResizeCntOld, sizeof c, hipMemcpyDeviceToHost, ctx->st));
    HIPCK(hipStreamSynchronize(ctx->st));
    *entries = c.entries;
    return 0;
}

extern "C" int hdrf_index_info_get(hdrf_ctx *ctx, hdrf_index_info *out)
{
    HDRF_LOCK(ctx);
    if (!ctx || !out) return HDRF_E_INVAL;
    if (int rc = drain(ctx)) return rc;
    uint64_t entries = 0;
    if (int rc = count_live(ctx, &entries, nullptr)) return rc;
    hdrf_index_info I{};
    I.index_log2 = ctx->cfg.index_log2;
    I.slots = (int64_t)1 << I.index_log2;
    I.entries = (int64_t)entries;
    I.table_bytes = I.slots * (int64_t)sizeof(IndexEntry);
    *out = I;
    return 0;
}

extern "C" int hdrf_index_resize(hdrf_ctx *ctx, int32_t new_log2)
{
    HDRF_LOCK(ctx);
    if (!ctx) return HDRF_E_INVAL;
    if (ctx->G > 1) return set_err(ctx, HDRF_E_UNSUPPORTED, "table resize on node-global contexts");
    if (!resize_log2_ok(new_log2)) return set_err(ctx, HDRF_E_INVAL, "hdrf_index_resize: new_log2 outside [10, 31]");
    if (int rc = drain(ctx)) return rc;
    const int old_log2 = ctx->cfg.index_log2;
    if (resize_check_args(old_log2, new_log2) == kResizeSame) return 0;
    hipStream_t st = ctx->st;
    StageTimer tm("HDRF_RESIZE_TIMES", 6);               // count / clear / rehash / count: scripts/index_resize_speed.py
    uint64_t entries = 0;
    if (int rc = count_live(ctx, &entries, &tm)) return rc;
    if (resize_check(old_log2, new_log2, entries) == kResizeTooFull)
        return set_err(ctx, HDRF_E_CAPACITY, "hdrf_index_resize: " + std::to_string(entries) + " entries would load a table of 2^" +
                                                 std::to_string(new_log2) + " slots past 75 %");
    IndexEntry *nt = nullptr;
    if (hipMalloc((void **)&nt, sizeof(IndexEntry) << new_log2) != hipSuccess) {
        (void)hipGetLastError();
        return set_err(ctx, HDRF_E_NOMEM, "hdrf_index_resize: no memory for a table of 2^" + std::to_string(new_log2) +
                                              " slots (both tables are resident during the call)");
    }
    // From here to the swap the old table is only read, and every failure frees the new one.
    uint8_t *R = ctx->d_rd;
    GcCounters after{};
    uint32_t rerr = 0;
    tm.mark(2, st);
    hipError_t e = launch_index_clear(nt, new_log2, nullptr, AllocState{}, st);     // (no allocator: it stays as it is)
    tm.mark(3, st);
    if (e == hipSuccess) e = hipMemsetAsync(R + kResizeErr, 0, 4, st);
    if (e == hipSuccess)
        e = launch_index_rehash(ctx->d_tab, old_log2, tag_mask(ctx), nt, new_log2, (uint32_t *)(R + kResizeErr), ctx->n_cu, st);
    tm.mark(4, st);
    if (e == hipSuccess) e = enqueue_count(ctx, nt, new_log2, kResizeCntNew);
    tm.mark(5, st);
    if (e == hipSuccess) e = hipMemcpyAsync(&after, R + kResizeCntNew, sizeof after, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(&rerr, R + kResizeErr, sizeof rerr, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        (void)hipFree(nt);
        return set_err(ctx, HDRF_E_HIP, std::string("hdrf_index_resize: ") + hipGetErrorString(e) + " (the index is unchanged)");
    }
    if (rerr || after.entries != entries) {
        (void)hipFree(nt);
        return set_err(ctx, HDRF_E_DEVICE, "hdrf_index_resize: " + std::to_string(after.entries) + " of " + std::to_string(entries) +
                                               " entries arrived in the new table" + (rerr ? " (it was full)" : "") +
                                               "; the index is unchanged");
    }
    IndexEntry *old = ctx->d_tab;
    ctx->d_tab = nt;
    ctx->cfg.index_log2 = new_log2;
    ctx->probe_stale = true;
    (void)hipFree(old);
    if (tm.on) {
        const ResizeBytes b = resize_bytes(old_log2, new_log2, entries);
        fprintf(stderr, "hdrf_index_resize times: count %.3f ms, clear %.3f ms, rehash %.3f ms, recount %.3f ms "
                        "(log2 %d -> %d, entries %llu, rehash bytes %llu)\n",
                tm.ms(0, 1), tm.ms(2, 3), tm.ms(3, 4), tm.ms(4, 5), old_log2, new_log2, (unsigned long long)entries,
                (unsigned long long)b.rehash());
    }
    return 0;
}
