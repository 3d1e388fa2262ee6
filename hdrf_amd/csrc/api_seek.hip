// api_seek.hip — libhdrf C-ABI: seek tables (hdrf_seek_build / _drop / _info_get; kernels in seek.hip,
// the arithmetic in seek_plan.hpp).  The reads that use the tables are api_views.hip's read_batch_body.
//
// hdrf_seek_build drains the pipeline, grows the read-side scratch (d_rd) and writes the seek store
// (schunks, scur, shead) and the table map (seeks); hdrf_seek_drop writes the map and, for all ids,
// frees the store.  Tables also leave in api.hip (recipe_alloc, reset_host, free_all) and api_gc.hip
// (hdrf_block_delete): host map operations, nothing is launched.
#include "ctx.hpp"
#include "seek_plan.hpp"

static_assert(sizeof(hdrf_seek_info) == 40, "hdrf_seek_info: ctypes mirror SeekInfo in hdrf_amd/lib.py");

constexpr uint64_t kSeekChunk = 64ull << 20;             // the seek store grows by chunks of this size

// space for a table of n chunks in the seek store (entries start on 16 B)
static int seek_alloc(hdrf_ctx *ctx, uint32_t n, hdrf_ctx::SeekLoc *loc)
{
    const uint64_t bytes = (uint64_t)n * 4;
    if (bytes > kSeekChunk) return set_err(ctx, HDRF_E_CAPACITY, "seek table larger than a seek-store chunk");
    if (ctx->scur < ctx->schunks.size() && ctx->shead + bytes > kSeekChunk) { ctx->scur++; ctx->shead = 0; }
    if (ctx->scur >= ctx->schunks.size()) {
        uint8_t *p = nullptr;
        if (hipMalloc((void **)&p, kSeekChunk) != hipSuccess) {
            (void)hipGetLastError();
            return set_err(ctx, HDRF_E_NOMEM, "hipMalloc failed (seek store)");
        }
        ctx->schunks.push_back(p);
        ctx->scur = (uint32_t)ctx->schunks.size() - 1;
        ctx->shead = 0;
    }
    *loc = hdrf_ctx::SeekLoc{ctx->scur, ctx->shead, n, 0};
    ctx->shead += (bytes + 15) & ~15ull;
    return 0;
}

// One group of ids: a zero-length request per stored recipe through rv_lookup + rv_scan, which leave
// off and len per chunk and fail an id whose digest is absent or whose lengths do not add up; then
// sk_store.  res[i] (i in [g0, g1)) is filled; the group's tables join the map.
static int seek_build_group(hdrf_ctx *ctx, const uint64_t *ids, int64_t g0, int64_t g1, std::vector<int> &res)
{
    std::vector<ReadDesc> desc;
    std::vector<hdrf_ctx::SeekLoc> loc;
    std::vector<uint64_t> dst;
    std::vector<int64_t> who;                            // desc row -> index in ids
    ReadPrefix px;
    for (int64_t i = g0; i < g1; i++) {
        const uint32_t key = (uint32_t)ids[i];
        ctx->seeks.erase(key);                           // rebuilt below, or gone
        auto it = ctx->recipes.find(key);
        if (it == ctx->recipes.end()) { res[(size_t)i] = HDRF_E_NOTFOUND; continue; }
        const uint64_t size = (uint64_t)ctx->lengths[key];
        if (it->second.n == 0 && size != 0) { res[(size_t)i] = HDRF_E_DEVICE; continue; }   // a recipe without digests
        hdrf_ctx::SeekLoc l{};
        if (int rc = seek_alloc(ctx, it->second.n, &l)) return rc;
        ReadDesc d{};
        d.dig = (uint64_t)(uintptr_t)(ctx->rchunks[it->second.chunk] + it->second.off);
        d.n = it->second.n;
        d.size = (uint32_t)size;
        if (!px.add(d.n, 0, 0, kReadTile, &d.row0, &d.tile0))
            return set_err(ctx, HDRF_E_CAPACITY, "seek build: too many chunks for one group");
        desc.push_back(d);
        loc.push_back(l);
        dst.push_back((uint64_t)(uintptr_t)(ctx->schunks[l.chunk] + l.off));
        who.push_back(i);
    }
    const uint32_t m = (uint32_t)desc.size();
    if (m == 0) return 0;
    // [descriptors | container ids | bases | destinations, as read_layout's digest bytes] one upload;
    // then the status words, the rows, and behind them the minlen words
    const ReadLayout L = read_layout(m, 0, (uint64_t)m * 8, px.rows, (uint32_t)sizeof(RdChunk));
    const uint64_t o_min = L.total, total = L.total + read_up256((uint64_t)m * 4);
    if (int rc = grow(ctx, &ctx->d_rd, &ctx->rd_cap, total)) return rc == HDRF_E_HIP ? HDRF_E_NOMEM : rc;
    uint8_t *R = ctx->d_rd;
    std::vector<uint8_t> up(L.upload, 0);
    std::memcpy(up.data() + L.o_desc, desc.data(), desc.size() * sizeof(ReadDesc));
    std::memcpy(up.data() + L.o_dig, dst.data(), dst.size() * 8);
    hipStream_t st = ctx->st;
    std::vector<int> status(m, 0);
    std::vector<uint32_t> minlen(m, 0);
    HIPCK(hipMemcpyAsync(R, up.data(), up.size(), hipMemcpyHostToDevice, st));
    HIPCK(hipMemsetAsync(R + L.o_status, 0, (size_t)m * 4, st));
    HIPCK(hipMemsetAsync(R + o_min, 0xff, (size_t)m * 4, st));
    // no container list: the build needs only the index (a zero-length range touches no container)
    HIPCK(launch_readv(ctx->cfg.hasher, (const ReadDesc *)(R + L.o_desc), (int)m, (uint32_t)px.rows, 0, kReadTile, ctx->d_tab,
                       ctx->cfg.index_log2, tag_mask(ctx), (const uint32_t *)(R + L.o_cid), (const uint64_t *)(R + L.o_base), 0,
                       (RdChunk *)(R + L.o_rows), (int *)(R + L.o_status), st));
    HIPCK(launch_seek_store((const ReadDesc *)(R + L.o_desc), (int)m, (const RdChunk *)(R + L.o_rows),
                            (const int *)(R + L.o_status), (const uint64_t *)(R + L.o_dig), (uint32_t *)(R + o_min), st));
    HIPCK(hipMemcpyAsync(status.data(), R + L.o_status, (size_t)m * 4, hipMemcpyDeviceToHost, st));
    HIPCK(hipMemcpyAsync(minlen.data(), R + o_min, (size_t)m * 4, hipMemcpyDeviceToHost, st));
    HIPCK(hipStreamSynchronize(st));
    for (uint32_t r = 0; r < m; r++) {
        const int64_t i = who[r];
        const uint32_t key = (uint32_t)ids[i];
        if (status[r] & kReadNotFound) res[(size_t)i] = HDRF_E_NOTFOUND;
        else if (status[r] & kReadDevice) res[(size_t)i] = HDRF_E_DEVICE;
        else {
            loc[r].minlen = minlen[r];                   // (0xffffffff: a recipe of at most one chunk)
            ctx->seeks[key] = loc[r];
            res[(size_t)i] = 0;
        }
        if (res[(size_t)i]) ctx->seeks.erase(key);       // (the id may come twice in one call)
    }
    return 0;
}

extern "C" int hdrf_seek_build(hdrf_ctx *ctx, const uint64_t *block_ids, int32_t n, int32_t *result)
{
    HDRF_LOCK(ctx);
    if (!ctx || n < 0 || (n && !block_ids)) return HDRF_E_INVAL;
    if (ctx->G > 1) return set_err(ctx, HDRF_E_UNSUPPORTED, "seek tables on node-global contexts");
    if (int rc = drain(ctx)) return rc;                  // blocks in flight first: their recipes are SET
    std::vector<int> res((size_t)n, 0);
    std::vector<uint32_t> cnt((size_t)n, 0);
    for (int32_t i = 0; i < n; i++) {
        auto it = ctx->recipes.find((uint32_t)block_ids[i]);
        if (it != ctx->recipes.end()) cnt[(size_t)i] = it->second.n;
    }
    for (int64_t g0 = 0; g0 < n;) {
        const int64_t g1 = seek_group_end(cnt.data(), n, g0, HDRF_READ_MAX_REQS);
        if (int rc = seek_build_group(ctx, block_ids, g0, g1, res)) return rc;
        g0 = g1;
    }
    int first = 0;
    for (int32_t i = 0; i < n; i++) {
        if (result) result[i] = res[(size_t)i];
        if (res[(size_t)i] && !first)
            first = set_err(ctx, res[(size_t)i],
                            "seek build, block " + std::to_string(block_ids[i]) + ": " +
                                (res[(size_t)i] == HDRF_E_NOTFOUND
                                     ? "no recipe for this block (keep_recipes?), or a recipe digest is not in the index"
                                     : "chunk lengths do not add up to the recipe size"));
    }
    return first;
}

extern "C" int hdrf_seek_drop(hdrf_ctx *ctx, const uint64_t *block_ids, int32_t n)
{
    HDRF_LOCK(ctx);
    if (!ctx || (block_ids && n < 0)) return HDRF_E_INVAL;
    if (int rc = drain(ctx)) return rc;
    if (!block_ids) {
        ctx->seeks.clear();
        for (auto p : ctx->schunks) (void)hipFree(p);
        ctx->schunks.clear();
        ctx->scur = 0;
        ctx->shead = 0;
        return 0;
    }
    for (int32_t i = 0; i < n; i++) ctx->seeks.erase((uint32_t)block_ids[i]);
    return 0;
}

extern "C" int hdrf_seek_info_get(hdrf_ctx *ctx, hdrf_seek_info *out)
{
    HDRF_LOCK(ctx);
    if (!ctx || !out) return HDRF_E_INVAL;
    if (int rc = drain(ctx)) return rc;                  // (a pending hdrf_reset_async drops every table)
    hdrf_seek_info s{};
    s.blocks = (int64_t)ctx->seeks.size();
    for (auto &kv : ctx->seeks) s.chunks += kv.second.n;
    s.bytes = (int64_t)(ctx->schunks.size() * kSeekChunk);
    s.last_rows = ctx->seek_last_rows;
    s.last_seek_reqs = ctx->seek_last_reqs;
    *out = s;
    return 0;
}
