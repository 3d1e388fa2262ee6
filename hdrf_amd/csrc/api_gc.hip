// api_gc.hip — libhdrf C-ABI: block deletion (FsDatasetImpl.invalidate) and the index garbage
// collection that follows it (kernels in gc.hip, the flat-range arithmetic in gc_plan.hpp).
//
// hdrf_block_delete writes the recipe and length maps and stats.recipe_bytes.  hdrf_gc drains the
// pipeline, grows the read-side scratch (d_rd) and, unless HDRF_GC_DRY, writes the index table and the
// index generation (epoch, bfirst, batch) — and `lost` when the rebuild fails after the switch.
#include "ctx.hpp"
#include "gc_plan.hpp"

static_assert(sizeof(hdrf_gc_stats) == 80, "hdrf_gc_stats: ctypes mirror GcStats in hdrf_amd/lib.py");
static_assert(sizeof(hdrf_gc_container) == 40, "hdrf_gc_container: ctypes mirror GcContainer in hdrf_amd/lib.py");

extern "C" int hdrf_block_delete(hdrf_ctx *ctx, uint64_t block_id)
{
    HDRF_LOCK(ctx);
    if (!ctx) return HDRF_E_INVAL;
    if (int rc = drain(ctx)) return rc;                  // blocks in flight first: their recipes are SET
    const uint32_t key = (uint32_t)block_id;
    auto r = ctx->recipes.find(key);
    auto l = ctx->lengths.find(key);
    if (r == ctx->recipes.end() && l == ctx->lengths.end())
        return set_err(ctx, HDRF_E_NOTFOUND, "no block " + std::to_string(block_id));
    if (r != ctx->recipes.end()) {
        // (a recipe restored with hdrf_recipe_load was never added to the total)
        ctx->stats.recipe_bytes -= std::min<int64_t>(ctx->stats.recipe_bytes, 4 + (int64_t)r->second.n * ctx->H);
        ctx->recipes.erase(r);                           // its digests stay in the append-only recipe store
    }
    if (l != ctx->lengths.end()) ctx->lengths.erase(l);
    ctx->seeks.erase(key);                               // its seek table goes with it
    return 0;
}

extern "C" int64_t hdrf_gc(hdrf_ctx *ctx, int32_t flags, hdrf_gc_stats *st_out, hdrf_gc_container *rows, int64_t cap)
{
    HDRF_LOCK(ctx);
    if (!ctx) return HDRF_E_INVAL;
    if (cap < 0 || (cap && !rows) || (flags & ~HDRF_GC_DRY)) return set_err(ctx, HDRF_E_INVAL, "hdrf_gc: bad arguments");
    if (ctx->G > 1) return set_err(ctx, HDRF_E_UNSUPPORTED, "garbage collection on node-global contexts");
    if (!ctx->cfg.keep_recipes)
        return set_err(ctx, HDRF_E_INVAL, "hdrf_gc needs cfg.keep_recipes: the context's recipes are the live set");
    for (int i = 0; i < hdrf_ctx::kRx; i++)
        if (ctx->rx[i].state.load() == 1)
            return set_err(ctx, HDRF_E_INVAL, "a block is being received (hdrf_submit_slot or hdrf_rx_cancel first)");
    if (int rc = drain(ctx)) return rc;
    const bool dry = (flags & HDRF_GC_DRY) != 0;
    const int log2cap = ctx->cfg.index_log2, HW = ctx->HW;
    const uint64_t nslots = 1ull << log2cap;
    // the live set: one job per recipe
    GcPlan plan;
    for (auto &kv : ctx->recipes)
        plan.add((uint64_t)(uintptr_t)(ctx->rchunks[kv.second.chunk] + kv.second.off), kv.second.n);
    plan.finish();
    const uint64_t row_cap = dry ? 0 : gc_row_cap(plan.total, nslots);
    if (row_cap >= (1ull << 31)) return set_err(ctx, HDRF_E_CAPACITY, "hdrf_gc: too many survivor rows for one rebuild");
    // container ids: what the host knows; ids seen only in entries join after a first sweep
    std::set<uint32_t> idset;
    for (auto &kv : ctx->containers) idset.insert(kv.first);
    for (auto &kv : ctx->loaded) idset.insert(kv.first);
    hipStream_t st = ctx->st;
    StageTimer tm("HDRF_GC_TIMES", 5);                   // mark / sweep / rebuild: scripts/gc_speed.py
    GcCounters c{};
    GcLayout L{};
    std::vector<uint32_t> cids;
    uint8_t *R = nullptr;
    for (int pass = 0;; pass++) {
        cids.assign(idset.begin(), idset.end());
        const uint64_t ncont = cids.size();
        L = gc_layout(plan.njobs(), std::max<uint64_t>(1, ncont), nslots, row_cap, (uint32_t)HW, sizeof(GcContCount));
        if (int rc = grow(ctx, &ctx->d_rd, &ctx->rd_cap, L.total)) return rc == HDRF_E_HIP ? HDRF_E_NOMEM : rc;
        R = ctx->d_rd;
        HIPCK(hipMemcpyAsync(R + L.o_jobs, plan.jobs.data(), plan.jobs.size() * sizeof(GcJob), hipMemcpyHostToDevice, st));
        if (ncont) HIPCK(hipMemcpyAsync(R + L.o_cid, cids.data(), ncont * 4, hipMemcpyHostToDevice, st));
        HIPCK(hipMemsetAsync(R + L.o_cnt, 0, 256, st));
        HIPCK(hipMemsetAsync(R + L.o_ccnt, 0, L.o_dw - L.o_ccnt, st));     // container counters, id and mark bitmaps
        tm.mark(0, st);
        HIPCK(launch_gc_mark(ctx->cfg.hasher, (const GcJob *)(R + L.o_jobs), plan.njobs(), plan.total, ctx->d_tab, log2cap,
                             tag_mask(ctx), (uint32_t *)(R + L.o_mark), (GcCounters *)(R + L.o_cnt), st));
        tm.mark(1, st);
        HIPCK(launch_gc_sweep(ctx->cfg.hasher, ctx->d_tab, log2cap, tag_mask(ctx), (const uint32_t *)(R + L.o_mark),
                              (const uint32_t *)(R + L.o_cid), (int)ncont, (GcContCount *)(R + L.o_ccnt),
                              (uint32_t *)(R + L.o_seen), dry ? nullptr : (uint32_t *)(R + L.o_dw), R + L.o_val, row_cap,
                              (uint32_t *)(R + L.o_wg), (GcCounters *)(R + L.o_cnt), 4 * ctx->n_cu, st));
        tm.mark(2, st);
        HIPCK(hipMemcpyAsync(&c, R + L.o_cnt, sizeof c, hipMemcpyDeviceToHost, st));
        HIPCK(hipStreamSynchronize(st));
        if (c.err) return set_err(ctx, HDRF_E_DEVICE, "hdrf_gc: the sweep reported an inconsistency (" + std::to_string(c.err) + ")");
        if (!c.n_unknown) break;
        if (pass) return set_err(ctx, HDRF_E_DEVICE, "hdrf_gc: container ids outside the collected list");
        std::vector<uint32_t> seen(kGcCidBits / 32);
        HIPCK(hipMemcpy(seen.data(), R + L.o_seen, kGcCidBits / 8, hipMemcpyDeviceToHost));
        for (uint32_t wd = 0; wd < seen.size(); wd++)
            for (uint32_t v = seen[wd]; v; v &= v - 1) idset.insert(wd * 32 + (uint32_t)__builtin_ctz(v));
    }
    const size_t ncont = cids.size();
    std::vector<GcContCount> cc(ncont);
    if (ncont) HIPCK(hipMemcpy(cc.data(), R + L.o_ccnt, ncont * sizeof(GcContCount), hipMemcpyDeviceToHost));
    if (c.kept + c.dropped != c.entries || (!dry && (c.n_rows != c.kept || c.n_marked != c.kept)))
        return set_err(ctx, HDRF_E_DEVICE, "hdrf_gc: the sweep's counts disagree (kept + dropped != entries, or the "
                                           "survivor rows are not the kept entries); the index is unchanged");
    hdrf_gc_stats S{};
    S.recipes = (int64_t)plan.recipes;
    S.recipe_digests = (int64_t)plan.total;
    S.entries = (int64_t)c.entries;
    S.kept = (int64_t)c.kept;
    S.dropped = (int64_t)c.dropped;
    S.kept_bytes = (int64_t)c.kept_bytes;
    S.dropped_bytes = (int64_t)c.dropped_bytes;
    S.missing = (int64_t)c.missing;
    std::vector<hdrf_gc_container> out;                  // (cids is sorted)
    for (size_t i = 0; i < ncont; i++) {
        if (!cc[i].kept_chunks && !cc[i].dropped_chunks) continue;      // no entry names it
        hdrf_gc_container g{};
        g.id = cids[i];
        g.readable = ctx->containers.count(cids[i]) || ctx->loaded.count(cids[i]) ? 1 : 0;
        g.kept_chunks = (int64_t)cc[i].kept_chunks;
        g.kept_bytes = (int64_t)cc[i].kept_bytes;
        g.dropped_chunks = (int64_t)cc[i].dropped_chunks;
        g.dropped_bytes = (int64_t)cc[i].dropped_bytes;
        S.dead_containers += g.kept_chunks == 0;
        out.push_back(g);
    }
    S.containers = (int64_t)out.size();
    if (!dry) {
        // Rebuild.  The scratch is allocated and every check made: from here on the index changes.  A
        // fresh index is a new epoch (api.hip init_state): every entry of the old one is empty, the
        // table is really cleared only when the epoch wraps, and the kept entries are restored into
        // it by the restore's kernel (hdrf_index_load).  The allocator is left as it is.
        AllocState cur{};
        HIPCK(hipMemcpy(&cur, ctx->d_alloc, sizeof cur, hipMemcpyDeviceToHost));
        const bool clear = ctx->epoch >= 255;
        ctx->epoch = clear ? 1 : ctx->epoch + 1;
        ctx->bfirst = ctx->batch + 1;
        int *d_err = (int *)(R + L.o_cnt + 128);
        GcCounters after{};
        int lerr = 0;
        tm.mark(3, st);
        hipError_t e = clear ? launch_index_clear(ctx->d_tab, log2cap, ctx->d_alloc, cur, st) : hipSuccess;
        if (e == hipSuccess) e = hipMemsetAsync(R + L.o_cnt, 0, 256, st);
        if (e == hipSuccess)
            e = launch_index_load(ctx->cfg.hasher, (const uint32_t *)(R + L.o_dw), R + L.o_val, (int)c.kept, ctx->d_tab,
                                  log2cap, tag_mask(ctx), ++ctx->batch, d_err, st);
        tm.mark(4, st);
        if (e == hipSuccess)                             // the inserted count: the live entries of the new epoch
            e = launch_gc_sweep(ctx->cfg.hasher, ctx->d_tab, log2cap, tag_mask(ctx), nullptr, nullptr, 0, nullptr, nullptr,
                                nullptr, nullptr, 0, nullptr, (GcCounters *)(R + L.o_cnt), 4 * ctx->n_cu, st);
        if (e == hipSuccess) e = hipMemcpyAsync(&after, R + L.o_cnt, sizeof after, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(&lerr, d_err, sizeof lerr, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) {
            ctx->lost = true;
            return set_err(ctx, HDRF_E_HIP, std::string("hdrf_gc rebuild: ") + hipGetErrorString(e) + " (hdrf_reset)");
        }
        if (lerr || after.entries != c.kept) {
            ctx->lost = true;
            return set_err(ctx, HDRF_E_DEVICE, "hdrf_gc rebuild: " + std::to_string(after.entries) + " of " +
                                                   std::to_string(c.kept) + " kept entries inserted (hdrf_reset)");
        }
    }
    if (tm.on) {
        fprintf(stderr, "hdrf_gc times: mark %.3f ms, sweep %.3f ms, rebuild %.3f ms (entries %lld, kept %lld, digests %lld)\n",
                tm.ms(0, 1), tm.ms(1, 2), dry ? 0.f : tm.ms(3, 4),
                (long long)S.entries, (long long)S.kept, (long long)S.recipe_digests);
    }
    const int64_t nout = std::min<int64_t>(cap, (int64_t)out.size());
    if (nout) std::memcpy(rows, out.data(), (size_t)nout * sizeof(hdrf_gc_container));
    if (st_out) *st_out = S;
    return (int64_t)out.size();
}
