// api_views.hip — libhdrf C-ABI: what a DataNode reads back or restores once batches have completed:
// index views, restore (index, allocator, recipes), recipes and block lengths, container read / load /
// unload, the durable-container drain, reconstruction, and the batched ranged reads.
//
// The views drain the pipeline and write nothing but the grown scratch buffers (d_rd, d_stage).
// Restore writes the index table, the allocator (d_alloc, h_alloc, have_alloc), containers and
// recipes; load / unload write ctx->loaded; hdrf_drain_containers writes the drain bookkeeping
// (pend_closed, undrained, handed) and the drain job list (h_xfer).
#include "ctx.hpp"
#include "read_plan.hpp"
#include "seek_plan.hpp"

// ---- index views ------------------------------------------------------------------------
// an entry's digest bytes (index_entry.hpp: the words are little-endian loads of them)
static void entry_digest(const IndexEntry &e, int H, uint8_t *out)
{
    uint32_t dw[7];
    if (H == 20) entry_digest_words<5>(e.tag, e.ncopy, e.dig, dw);
    else entry_digest_words<7>(e.tag, e.ncopy, e.dig, dw);
    std::memcpy(out, dw, (size_t)H);
}

extern "C" int hdrf_index_get(hdrf_ctx *ctx, const uint8_t *digest, uint8_t out11[11])
{
    HDRF_LOCK(ctx);
    if (!ctx || !digest) return HDRF_E_INVAL;
    uint32_t dw[2];
    std::memcpy(dw, digest, 8);
    const unsigned long long key = tag_mask(ctx), tag = tag_word(dw, key);
    const uint64_t mask = (1ull << ctx->cfg.index_log2) - 1;
    uint64_t h = tag_home(tag, ctx->cfg.index_log2);
    if (int rc = drain(ctx)) return rc;
    for (uint64_t probe = 0; probe <= mask; probe++) {
        IndexEntry e;
        HIPCK(hipMemcpy(&e, ctx->d_tab + h, sizeof e, hipMemcpyDeviceToHost));
        if (!tag_live(e.tag, key)) return 0;
        uint8_t full[28];
        entry_digest(e, ctx->H, full);
        if (e.tag == tag && std::memcmp(full, digest, ctx->H) == 0) {
            if (out11) encode_value(e.ncopy, e.cid, e.start, e.stop, out11);
            return 1;
        }
        h = (h + 1) & mask;
    }
    return 0;
}

static int fetch_table(hdrf_ctx *ctx, std::vector<IndexEntry> &tab)
{
    tab.resize((size_t)1 << ctx->cfg.index_log2);
    if (int rc = drain(ctx)) return rc;
    HIPCK(hipMemcpy(tab.data(), ctx->d_tab, tab.size() * sizeof(IndexEntry), hipMemcpyDeviceToHost));
    return 0;
}

// Probe lengths of the last completed batch (linear probing from each chunk's home slot to the
// entry it resolved to): sum, max and the number of chunks.  Steady-state index measurement.
extern "C" int hdrf_probe_stats(hdrf_ctx *ctx, int64_t *probe_sum, int64_t *probe_max, int64_t *chunks)
{
    HDRF_LOCK(ctx);
    if (!ctx || !probe_sum || !probe_max || !chunks) return HDRF_E_INVAL;
    if (ctx->G > 1) return set_err(ctx, HDRF_E_UNSUPPORTED, "probe stats on node-global contexts");
    if (int rc = drain(ctx)) return rc;
    Slot &S = ctx->sl[ctx->res];
    if (ctx->last_nblocks < 1) return set_err(ctx, HDRF_E_INVAL, "no completed batch");
    if (ctx->probe_stale) {                              // the batch's slots are those of the table before a resize
        *probe_sum = *probe_max = *chunks = 0;
        return 0;
    }
    unsigned long long *d = nullptr;
    HIPCK(hipMalloc((void **)&d, 3 * sizeof(unsigned long long)));
    unsigned long long h[3] = {0, 0, 0};
    hipError_t e = hipMemsetAsync(d, 0, sizeof h, ctx->st);
    if (e == hipSuccess)
        e = launch_index_probe(ctx->cfg.hasher, S.d_bst, ctx->last_nblocks, ctx->cap_blk, S.d_dig, S.d_slot,
                               ctx->cfg.index_log2, tag_mask(ctx), d, ctx->st);
    if (e == hipSuccess) e = hipMemcpyAsync(h, d, sizeof h, hipMemcpyDeviceToHost, ctx->st);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->st);
    (void)hipFree(d);
    if (e != hipSuccess) return set_err(ctx, HDRF_E_HIP, hipGetErrorString(e));
    *probe_sum = (int64_t)h[0];
    *probe_max = (int64_t)h[1];
    *chunks = (int64_t)h[2];
    return 0;
}

extern "C" int64_t hdrf_index_count(hdrf_ctx *ctx)
{
    HDRF_LOCK(ctx);
    if (!ctx) return HDRF_E_INVAL;
    std::vector<IndexEntry> tab;
    if (int rc = fetch_table(ctx, tab)) return rc;
    int64_t n = 0;
    const unsigned long long key = tag_mask(ctx);
    for (auto &e : tab) n += tag_live(e.tag, key);
    return n;
}

extern "C" int64_t hdrf_index_dump(hdrf_ctx *ctx, uint8_t *keys, uint8_t *vals, int64_t cap)
{
    HDRF_LOCK(ctx);
    if (!ctx) return HDRF_E_INVAL;
    std::vector<IndexEntry> tab;
    if (int rc = fetch_table(ctx, tab)) return rc;
    const int H = ctx->H;
    std::vector<std::vector<uint8_t>> rows;
    const unsigned long long key = tag_mask(ctx);
    for (auto &e : tab) {
        if (!tag_live(e.tag, key)) continue;
        std::vector<uint8_t> r(H + 11);
        entry_digest(e, H, r.data());
        encode_value(e.ncopy, e.cid, e.start, e.stop, r.data() + H);
        rows.push_back(std::move(r));
    }
    if ((int64_t)rows.size() > cap) return set_err(ctx, HDRF_E_CAPACITY, "index dump capacity");
    std::sort(rows.begin(), rows.end(),
              [H](const std::vector<uint8_t> &a, const std::vector<uint8_t> &b) { return std::memcmp(a.data(), b.data(), H) < 0; });
    for (size_t i = 0; i < rows.size(); i++) {
        std::memcpy(keys + i * H, rows[i].data(), H);
        std::memcpy(vals + i * 11, rows[i].data() + H, 11);
    }
    return (int64_t)rows.size();
}

extern "C" int hdrf_allocator(hdrf_ctx *ctx, uint8_t out24[24])
{
    HDRF_LOCK(ctx);
    if (!ctx || !out24) return HDRF_E_INVAL;
    if (!ctx->have_alloc) return 0;
    uint32_t v[8];
    for (int t = 0; t < 4; t++) {
        v[t] = ctx->h_alloc.id[t];
        v[t + 4] = ctx->h_alloc.pos[t];
    }
    for (int i = 0; i < 8; i++) {                   // utilities.blockIDtoBytes (DN/utilities.java:66-75)
        out24[3 * i] = (uint8_t)(v[i] >> 16);
        out24[3 * i + 1] = (uint8_t)(v[i] >> 8);
        out24[3 * i + 2] = (uint8_t)v[i];
    }
    return 1;
}

// ---- restore (index persistence: a DataNode restarting on its Redis dump + chunkDir) -------
// SET digest -> value for n entries (the rows of hdrf_index_dump) on a context whose index does
// not hold these digests yet (a fresh or reset context).
extern "C" int hdrf_index_load(hdrf_ctx *ctx, const uint8_t *keys, const uint8_t *vals, int64_t n)
{
    HDRF_LOCK(ctx);
    if (!ctx || n < 0 || (n && (!keys || !vals))) return HDRF_E_INVAL;
    if (ctx->G > 1) return set_err(ctx, HDRF_E_UNSUPPORTED, "restore on node-global contexts: not yet");
    if (int rc = drain(ctx)) return rc;
    if (n == 0) return 0;
    const uint64_t o_dw = 0, dw_b = (uint64_t)n * ctx->HW * 4;
    const uint64_t o_v = (dw_b + 255) & ~255ull, o_err = (o_v + (uint64_t)n * 11 + 255) & ~255ull;
    if (int rc = grow(ctx, &ctx->d_rd, &ctx->rd_cap, o_err + 256)) return rc;
    uint8_t *R = ctx->d_rd;
    hipStream_t st = ctx->st;
    std::vector<uint8_t> dw(dw_b, 0);                  // digest bytes as u32 words (SHA-224: 28 B)
    for (int64_t k = 0; k < n; k++) std::memcpy(dw.data() + (size_t)k * ctx->HW * 4, keys + (size_t)k * ctx->H, ctx->H);
    HIPCK(hipMemcpyAsync(R + o_dw, dw.data(), dw_b, hipMemcpyHostToDevice, st));
    HIPCK(hipMemcpyAsync(R + o_v, vals, (size_t)n * 11, hipMemcpyHostToDevice, st));
    HIPCK(hipMemsetAsync(R + o_err, 0, 4, st));
    HIPCK(launch_index_load(ctx->cfg.hasher, (const uint32_t *)(R + o_dw), R + o_v, (int)n, ctx->d_tab,
                            ctx->cfg.index_log2, tag_mask(ctx), ++ctx->batch, (int *)(R + o_err), st));
    int err = 0;
    HIPCK(hipMemcpyAsync(&err, R + o_err, 4, hipMemcpyDeviceToHost, st));
    HIPCK(hipStreamSynchronize(st));
    if (err) return set_err(ctx, HDRF_E_CAPACITY, "index table full (index_log2 too small)");
    return 0;
}

// SET "blockID" (the 24-B allocator, DN/utilities.java:66-75) and reopen the three storer
// ranges' open containers from their chunkDir files (open_len[t] < 0: no file): the storer
// appends to them exactly as threadedStorer does after reading prevData (:723-737).
extern "C" int hdrf_allocator_load(hdrf_ctx *ctx, const uint8_t alloc24[24], const uint8_t *const *open_files,
                                   const int64_t *open_len)
{
    HDRF_LOCK(ctx);
    if (!ctx || !alloc24 || !open_len) return HDRF_E_INVAL;
    if (ctx->G > 1) return set_err(ctx, HDRF_E_UNSUPPORTED, "restore on node-global contexts: not yet");
    if (int rc = drain(ctx)) return rc;
    AllocState a{};
    for (int i = 0; i < 8; i++) {
        const uint32_t v = ((uint32_t)alloc24[3 * i] << 16) | ((uint32_t)alloc24[3 * i + 1] << 8) | alloc24[3 * i + 2];
        if (i < 4) a.id[i] = v; else a.pos[i - 4] = v;
    }
    for (int t = 0; t < 4; t++) a.slot[t] = (uint32_t)t * (uint32_t)(ctx->cfg.arena_slots / 4);
    for (int t = 0; t < ctx->cfg.n_thread; t++) {
        if (open_len[t] < 0) continue;
        if ((uint64_t)open_len[t] > ctx->cfg.container_max || (open_len[t] && (!open_files || !open_files[t])))
            return set_err(ctx, HDRF_E_INVAL, "bad open container file");
        if (open_len[t])
            HIPCK(hipMemcpy(ctx->d_arena + (size_t)a.slot[t] * ctx->cfg.container_max, open_files[t],
                            (size_t)open_len[t], hipMemcpyHostToDevice));
        a.cur[t] = (uint32_t)open_len[t];
        a.exists[t] = 1;
    }
    HIPCK(hipMemcpy(ctx->d_alloc, &a, sizeof a, hipMemcpyHostToDevice));
    ctx->h_alloc = a;
    ctx->have_alloc = 1;
    for (int t = 0; t < ctx->cfg.n_thread; t++)
        if (a.exists[t]) note_container(ctx, a.id[t], a.slot[t], a.cur[t], 0);
    return 0;
}

// SET longToBytes(blockId,4) -> recipe (storeDB, DN/DataDeduplicator.java:372-392)
extern "C" int hdrf_recipe_load(hdrf_ctx *ctx, uint64_t block_id, const uint8_t *recipe, int64_t len)
{
    HDRF_LOCK(ctx);
    if (!ctx || !recipe || len < 4 || (len - 4) % ctx->H) return HDRF_E_INVAL;
    const uint32_t key = (uint32_t)block_id;
    if (int rc = drain(ctx)) return rc;
    const uint32_t n = (uint32_t)((len - 4) / ctx->H);
    uint8_t *dst = nullptr;
    if (int rc = recipe_alloc(ctx, (uint64_t)n * ctx->H, key, n, &dst)) return rc;
    if (n) HIPCK(hipMemcpy(dst, recipe + 4, (size_t)n * ctx->H, hipMemcpyHostToDevice));
    ctx->lengths[key] = ((int64_t)recipe[0] << 24) | (recipe[1] << 16) | (recipe[2] << 8) | recipe[3];
    return 0;
}

extern "C" int64_t hdrf_recipe_get(hdrf_ctx *ctx, uint64_t block_id, uint8_t *out, int64_t cap)
{
    HDRF_LOCK(ctx);
    if (!ctx) return HDRF_E_INVAL;
    if (int rc = drain(ctx)) return rc;                 // blocks in flight first: their recipes are SET
    auto it = ctx->recipes.find((uint32_t)block_id);
    if (it == ctx->recipes.end()) return 0;
    const int64_t n = 4 + (int64_t)it->second.n * ctx->H;
    if (!out || cap < n) return set_err(ctx, HDRF_E_CAPACITY, "recipe needs " + std::to_string(n) + " bytes");
    std::vector<uint8_t> r;
    const int fr = fetch_recipe(ctx, (uint32_t)block_id, r);
    if (fr < 0) return fr;
    std::memcpy(out, r.data(), (size_t)n);
    return n;
}

extern "C" int64_t hdrf_block_length(hdrf_ctx *ctx, uint64_t block_id)
{
    HDRF_LOCK(ctx);
    if (!ctx) return HDRF_E_INVAL;
    auto it = ctx->lengths.find((uint32_t)block_id);
    return it == ctx->lengths.end() ? HDRF_E_NOTFOUND : it->second;
}

extern "C" int64_t hdrf_container_read(hdrf_ctx *ctx, uint32_t id, uint8_t *out, int64_t cap, int32_t *closed)
{
    HDRF_LOCK(ctx);
    if (!ctx) return HDRF_E_INVAL;
    if (int rc = drain(ctx)) return rc;                 // batches in flight may append, close or recycle it
    auto it = ctx->containers.find(id);
    if (it == ctx->containers.end()) return set_err(ctx, HDRF_E_NOTFOUND, "container not resident");
    if (closed) *closed = it->second.closed;
    const bool lz = ctx->cfg.compressor == 2 && it->second.closed;     // the file is the Lz4Codec stream
    const int64_t n = lz ? it->second.clen : it->second.len;
    if (!out) return n;
    if (cap < n) return set_err(ctx, HDRF_E_CAPACITY, "container capacity");
    const uint8_t *src = lz ? ctx->d_carena + (size_t)it->second.slot * ctx->cslot
                            : ctx->d_arena + (size_t)it->second.slot * ctx->cfg.container_max;
    if (n) HIPCK(hipMemcpy(out, src, n, hipMemcpyDeviceToHost));
    return n;
}

// Make container `id` readable for reconstruction from its chunkDir file (raw, or a closed
// container's Lz4Codec file): a DataNode that restarted, or whose arena slot was reused.
extern "C" int hdrf_container_load(hdrf_ctx *ctx, uint32_t id, const uint8_t *file, int64_t flen, int32_t lz4)
{
    HDRF_LOCK(ctx);
    if (!ctx || flen < 0 || (flen && !file)) return HDRF_E_INVAL;
    uint64_t raw = (uint64_t)flen;
    if (lz4) {
        std::vector<LzDec> items;
        if (!plan_lz4_frame(file, flen, items, &raw)) return set_err(ctx, HDRF_E_INVAL, "malformed Lz4Codec frame");
    }
    if (raw > ctx->cfg.container_max) return set_err(ctx, HDRF_E_INVAL, "container larger than container_max");
    if (int rc = drain(ctx)) return rc;
    uint8_t *p = nullptr;
    HIPCK(hipMalloc((void **)&p, raw + 64));
    int64_t got = (int64_t)raw;
    if (lz4) got = decode_file(ctx, file, flen, p, (int64_t)raw);
    else if (raw) {
        if (hipMemcpy(p, file, raw, hipMemcpyHostToDevice) != hipSuccess) got = set_err(ctx, HDRF_E_HIP, "H2D copy");
    }
    if (got < 0) { (void)hipFree(p); return (int)got; }
    auto it = ctx->loaded.find(id);
    if (it != ctx->loaded.end()) (void)hipFree(it->second.ptr);
    ctx->loaded[id] = hdrf_ctx::Loaded{p, raw};
    return 0;
}

extern "C" int hdrf_container_unload(hdrf_ctx *ctx, uint32_t id)
{
    HDRF_LOCK(ctx);
    if (!ctx) return HDRF_E_INVAL;
    if (int rc = drain(ctx)) return rc;
    auto it = ctx->loaded.find(id);
    if (it == ctx->loaded.end()) return set_err(ctx, HDRF_E_NOTFOUND, "container not loaded");
    (void)hipFree(it->second.ptr);
    ctx->loaded.erase(it);
    return 0;
}

// ---- durable containers: the chunkDir files of the storers (DN/DataDeduplicator.java:748-818) ----
// Since the last drain: every container that closed (the whole file: raw bytes, or the Lz4Codec
// stream under compressor 2, rewritten at :748-786) in close order, then every open container's
// bytes appended since (:806-818).  Events are emitted whole, in order, while they fit.  Only what
// the COMPLETED batches (hdrf_wait_batch) produced is handed out; batches still in flight keep
// running: their place kernels only append past the bytes copied here, and a closed container's
// slot stays retained until it is drained.  The D2H copies run on stream D, so they overlap the
// H2D copies of later batches on stream C (PCIe is full duplex).
extern "C" int64_t hdrf_drain_containers(hdrf_ctx *ctx, hdrf_container_event *ev, int64_t ev_cap, uint8_t *out,
                                         int64_t out_cap, int64_t *need)
{
    HDRF_LOCK(ctx);
    if (!ctx) return HDRF_E_INVAL;
    if (need) *need = 0;
    if (!ctx->cfg.retain_containers) return set_err(ctx, HDRF_E_INVAL, "hdrf_drain_containers needs cfg.retain_containers");
    if (ctx->G > 1) return set_err(ctx, HDRF_E_UNSUPPORTED, "container drain on node-global contexts");
    if (ev_cap < 0 || out_cap < 0 || (ev_cap && !ev) || (out_cap && !out)) return set_err(ctx, HDRF_E_INVAL, "bad buffers");
    const hdrf_cfg &c = ctx->cfg;
    struct Pend { uint32_t id; int closed; int64_t off, n; ContainerInfo ci; };
    std::vector<Pend> todo;
    for (uint32_t id : ctx->pend_closed) {
        auto it = ctx->containers.find(id);
        if (it == ctx->containers.end()) return set_err(ctx, HDRF_E_DEVICE, "undrained container missing");
        if (c.compressor == 2) {                          // the whole Lz4Codec file replaces the raw one
            todo.push_back(Pend{id, 1, 0, (int64_t)it->second.clen, it->second});
        } else {
            // the storer's close rewrites the file as prevData || buffer (:754-786): the bytes already
            // handed out plus the rest, so only the rest travels (file_off = the bytes handed out)
            const int64_t done = ctx->handed.count(id) ? ctx->handed[id] : 0;
            todo.push_back(Pend{id, 1, done, (int64_t)it->second.len - done, it->second});
        }
    }
    const size_t nclosed = todo.size();
    for (int t = 0; t < c.n_thread; t++) {
        if (!ctx->h_alloc.exists[t]) continue;
        const uint32_t id = ctx->h_alloc.id[t];
        auto it = ctx->containers.find(id);
        if (it == ctx->containers.end()) continue;
        const int64_t done = ctx->handed.count(id) ? ctx->handed[id] : 0;
        if ((int64_t)it->second.len > done) todo.push_back(Pend{id, 0, done, (int64_t)it->second.len - done, it->second});
    }
    // pinned (device-mapped) output: the CUs write it (xfer_kernel), beside the SDMA H2D of later
    // batches (whole blocks through hdrf_submit_host: 38.8 / 39.1 vs 34.7 / 35.5 GB/s with the copy
    // engine); once the context receives packets (hdrf_rx_begin), the copy engine (22.0 vs 28.3 GB/s
    // for 64 KiB packets, profiles/r03_c5_drain_ab.txt); pageable output: hipMemcpyAsync.
    // HDRF_DRAIN_KERNEL=1 / 0 forces the CUs / the copy engine.
    static const int kern_env = [] { const char *e = getenv("HDRF_DRAIN_KERNEL"); return e ? (atoi(e) != 0) : -1; }();
    const bool kern = kern_env >= 0 ? kern_env != 0 : !ctx->rx_used;
    hipPointerAttribute_t pa;
    const bool mapped = kern && out_cap > 0 && hipPointerGetAttributes(&pa, out) == hipSuccess &&
                        pa.type == hipMemoryTypeHost && pa.devicePointer != nullptr;
    (void)hipGetLastError();
    if (mapped && ctx->xfer_cap == 0) {
        HIPCK(hipHostMalloc((void **)&ctx->h_xfer, sizeof(XferJob) * 1024, hipHostMallocDefault));
        ctx->xfer_cap = 1024;
    }
    int64_t k = 0, used = 0;
    int nj = 0;
    uint64_t maxj = 0;
    // CU drain grid: one workgroup per ~256 MiB of this drain, at least 5.  Five workgroups still drain
    // a config-5 batch in ~19.5 ms, but the next blocks' H2D copies beside them keep 54.9 GB/s, where
    // a full grid's flood of PCIe writes cut them to 44.6 (config 5 whole blocks: 50.0 / 50.1 GB/s
    // with 5 workgroups, 49.8 / 48.5 with 4, 41.5 with 3, 47.3 / 47.4 with one per item;
    // profiles/r04_drain_wgs_ab.txt, r04_c5_trace3.txt).  HDRF_XFER_WGS = W overrides (0: one per item).
    static const int wgs_env = env_int("HDRF_XFER_WGS", -1);
    int64_t drain_bytes = 0;
    for (const Pend &e : todo) drain_bytes += e.n;
    const int wgs = wgs_env >= 0 ? wgs_env : (int)std::max<int64_t>(5, (drain_bytes + (256ll << 20) - 1) / (256ll << 20));
    for (const Pend &e : todo) {
        if (k >= ev_cap || used + e.n > out_cap) {
            if (need) *need = e.n;
            break;
        }
        const uint8_t *src = (e.closed && c.compressor == 2) ? ctx->d_carena + (size_t)e.ci.slot * ctx->cslot
                                                             : ctx->d_arena + (size_t)e.ci.slot * c.container_max;
        if (e.n && mapped) {
            if (nj == ctx->xfer_cap) {                    // job list full: flush it
                HIPCK(launch_xfer(ctx->h_xfer, nj, maxj, wgs, ctx->stD));
                HIPCK(hipStreamSynchronize(ctx->stD));
                nj = 0;
                maxj = 0;
            }
            ctx->h_xfer[nj++] = XferJob{(uint64_t)(uintptr_t)(src + e.off),
                                        (uint64_t)(uintptr_t)((uint8_t *)pa.devicePointer + used), (uint64_t)e.n};
            maxj = std::max<uint64_t>(maxj, (uint64_t)e.n);
        } else if (e.n) {
            HIPCK(hipMemcpyAsync(out + used, src + e.off, (size_t)e.n, hipMemcpyDeviceToHost, ctx->stD));
        }
        ev[k] = hdrf_container_event{e.id, e.closed, e.off, e.n, used};
        used += e.n;
        k++;
    }
    if (nj) HIPCK(launch_xfer(ctx->h_xfer, nj, maxj, wgs, ctx->stD));
    HIPCK(hipStreamSynchronize(ctx->stD));
    // the emitted ones are handed over
    const size_t kc = std::min<size_t>((size_t)k, nclosed);
    for (size_t i = 0; i < kc; i++) {
        const uint32_t id = ctx->pend_closed[i];
        ctx->undrained[std::min<uint32_t>(id >> 22, 3)]--;
        ctx->handed.erase(id);
    }
    ctx->pend_closed.erase(ctx->pend_closed.begin(), ctx->pend_closed.begin() + kc);
    for (size_t i = nclosed; i < (size_t)k; i++) ctx->handed[todo[i].id] = todo[i].off + todo[i].n;
    if (k == 0 && !todo.empty()) return set_err(ctx, HDRF_E_CAPACITY, "drain buffer too small for the next event");
    return k;
}

// ---- read side: DataConstructor (DN/DataConstructor.java:73-250, 360-531) --------------------
int host::grow(hdrf_ctx *ctx, uint8_t **p, uint64_t *cap, uint64_t need)
{
    if (*cap >= need) return 0;
    if (*p) (void)hipFree(*p);
    *p = nullptr;
    *cap = 0;
    HIPCK(hipMalloc((void **)p, need));
    *cap = need;
    return 0;
}

// The containers a read can take bytes from, sorted by id: those loaded back from files, then the
// arena residents (which win on a tie), each with its base and its two bounds.
void host::readable_list(const hdrf_ctx *ctx, Readable &r)
{
    struct One { uint64_t base, alloc; uint32_t valid; };
    std::map<uint32_t, One> rdbl;
    for (auto &kv : ctx->loaded)                          // hdrf_container_load: raw + 64 bytes allocated
        rdbl[kv.first] = One{(uint64_t)(uintptr_t)kv.second.ptr, kv.second.len + 64, (uint32_t)kv.second.len};
    for (auto &kv : ctx->containers)
        rdbl[kv.first] = One{(uint64_t)(uintptr_t)(ctx->d_arena + (size_t)kv.second.slot * ctx->cfg.container_max),
                             ctx->cfg.container_max, kv.second.len};
    r.cid.clear(); r.base.clear(); r.alloc.clear(); r.valid.clear();
    for (auto &kv : rdbl) {
        r.cid.push_back(kv.first);
        r.base.push_back(kv.second.base);
        r.alloc.push_back(kv.second.alloc);
        r.valid.push_back(kv.second.valid);
    }
}

static std::string hex_digest(const uint8_t *d, int H)
{
    static const char *x = "0123456789abcdef";
    std::string s;
    for (int i = 0; i < H; i++) { s += x[d[i] >> 4]; s += x[d[i] & 15]; }
    return s;
}

// hdrf_reconstruct (bad_chunk == nullptr) and hdrf_reconstruct_verified: the caller holds the lock.
// Verified: once the gather ran, every chunk of the rebuilt block is re-hashed on the same stream and
// compared with its recipe digest (vf_hash, verify.hip), which checks the gather as well as the
// container bytes.
static int64_t reconstruct_body(hdrf_ctx *ctx, const uint8_t *recipe, int64_t recipe_len, uint8_t *dev_out, int64_t cap,
                                int64_t *bad_chunk)
{
    const bool verify = bad_chunk != nullptr;
    if (verify) *bad_chunk = -1;
    if (ctx->G > 1)
        return set_err(ctx, HDRF_E_UNSUPPORTED, "node-global contexts read through hdrf_gx_read_locate / _fill (every rank)");
    if (int rc = drain(ctx)) return rc;
    const int64_t size = ((int64_t)recipe[0] << 24) | (recipe[1] << 16) | (recipe[2] << 8) | recipe[3];
    const int64_t n = recipe_len / ctx->H;             // t1data.length / hash_length (:223)
    if (size > cap || (size && !dev_out)) return set_err(ctx, HDRF_E_CAPACITY, "output capacity");
    if (n == 0) return size == 0 ? 0 : set_err(ctx, HDRF_E_DEVICE, "recipe without digests");
    Readable rd;
    readable_list(ctx, rd);
    const std::vector<uint32_t> &cid = rd.cid;
    const std::vector<uint64_t> &base = rd.base;
    const int ncont = (int)cid.size();
    const uint64_t o_dig = 0, dig_b = (uint64_t)n * ctx->HW * 4;
    const uint64_t o_ch = (dig_b + 255) & ~255ull, ch_b = (uint64_t)n * sizeof(RdChunk);
    const uint64_t o_base = (o_ch + ch_b + 255) & ~255ull, base_b = (uint64_t)std::max(1, ncont) * 8;
    const uint64_t o_cid = (o_base + base_b + 255) & ~255ull, cid_b = (uint64_t)std::max(1, ncont) * 4;
    const uint64_t o_tot = (o_cid + cid_b + 255) & ~255ull;
    const uint64_t o_vf = o_tot + 64;                  // verified: the hash counters, in o_tot's 256 B
    static_assert(64 + sizeof(VfCounters) <= 256, "the counters share the totals' block");
    if (int rc = grow(ctx, &ctx->d_rd, &ctx->rd_cap, o_tot + 256)) return rc;
    uint8_t *R = ctx->d_rd;
    hipStream_t st = ctx->st;
    HIPCK(hipMemcpyAsync(R + o_dig, recipe + 4, (size_t)n * ctx->H, hipMemcpyHostToDevice, st));
    if (ncont) {
        HIPCK(hipMemcpyAsync(R + o_cid, cid.data(), cid.size() * 4, hipMemcpyHostToDevice, st));
        HIPCK(hipMemcpyAsync(R + o_base, base.data(), base.size() * 8, hipMemcpyHostToDevice, st));
    }
    HIPCK(hipMemsetAsync(R + o_tot, 0, 16, st));
    const uint64_t *bases = (const uint64_t *)(R + o_base);
    HIPCK(launch_reconstruct(ctx->cfg.hasher, (const uint32_t *)(R + o_dig), (int)n, ctx->d_tab, ctx->cfg.index_log2,
                             tag_mask(ctx), (const uint32_t *)(R + o_cid), bases, ncont, (RdChunk *)(R + o_ch),
                             (uint64_t *)(R + o_tot), dev_out, (int *)(R + o_tot + 8), st, false));
    uint64_t tot[2] = {0, 0};
    HIPCK(hipMemcpyAsync(tot, R + o_tot, 16, hipMemcpyDeviceToHost, st));
    HIPCK(hipStreamSynchronize(st));
    if ((int)tot[1]) return set_err(ctx, HDRF_E_NOTFOUND, "a recipe digest or its container is not readable");
    if ((int64_t)tot[0] != size) return set_err(ctx, HDRF_E_DEVICE, "chunk lengths do not add up to the recipe size");
    HIPCK(launch_reconstruct(ctx->cfg.hasher, nullptr, (int)n, nullptr, 0, 0, nullptr, bases, 0, (RdChunk *)(R + o_ch), nullptr,
                             dev_out, nullptr, st, true));
    VfCounters vc{};
    if (verify) {
        HIPCK(hipMemsetAsync(R + o_vf, 0, sizeof vc, st));
        HIPCK(launch_vf_hash_block(ctx->cfg.hasher, (const RdChunk *)(R + o_ch), (int)n, (const uint32_t *)(R + o_dig), dev_out,
                                   (uint64_t)size, (VfCounters *)(R + o_vf), vf_workgroups(ctx), st));
        HIPCK(hipMemcpyAsync(&vc, R + o_vf, sizeof vc, hipMemcpyDeviceToHost, st));
    }
    HIPCK(hipStreamSynchronize(st));
    if (verify && vc.checked != (uint32_t)n) return set_err(ctx, HDRF_E_DEVICE, "verified read: not every chunk was hashed");
    if (verify && vc.n_bad) {
        const uint32_t k = ~vc.first_bad_inv;
        *bad_chunk = k;
        RdChunk c{};
        HIPCK(hipMemcpy(&c, R + o_ch + (uint64_t)k * sizeof c, sizeof c, hipMemcpyDeviceToHost));
        const std::string where = c.slot < cid.size() ? "container " + std::to_string(cid[c.slot]) : std::string("no container");
        return set_err(ctx, HDRF_E_CORRUPT,
                       "recipe position " + std::to_string(k) + ": digest " + hex_digest(recipe + 4 + (size_t)k * ctx->H, ctx->H) +
                           ", " + where + " [" + std::to_string(c.start) + ", " + std::to_string(c.start + c.len) +
                           "): the bytes hash to another digest (" + std::to_string(vc.n_bad) + " of " +
                           std::to_string(n) + " chunks of the block)");
    }
    return size;
}

extern "C" int64_t hdrf_reconstruct(hdrf_ctx *ctx, const uint8_t *recipe, int64_t recipe_len, uint8_t *dev_out,
                                    int64_t cap)
{
    HDRF_LOCK(ctx);
    if (!ctx || !recipe || recipe_len < 4) return HDRF_E_INVAL;
    return reconstruct_body(ctx, recipe, recipe_len, dev_out, cap, nullptr);
}

extern "C" int64_t hdrf_reconstruct_verified(hdrf_ctx *ctx, const uint8_t *recipe, int64_t recipe_len, uint8_t *dev_out,
                                             int64_t cap, int64_t *bad_chunk)
{
    HDRF_LOCK(ctx);
    if (!ctx || !recipe || recipe_len < 4 || !bad_chunk) return HDRF_E_INVAL;
    return reconstruct_body(ctx, recipe, recipe_len, dev_out, cap, bad_chunk);
}

// hdrf_reconstruct_block (bad_chunk == nullptr) and hdrf_reconstruct_block_verified
static int64_t reconstruct_block_body(hdrf_ctx *ctx, uint64_t block_id, uint8_t *out, int64_t cap, int64_t *bad_chunk)
{
    if (bad_chunk) *bad_chunk = -1;
    if (int rc = drain(ctx)) return rc;
    std::vector<uint8_t> rec;                            // GET longToBytes(blockId,4) (DN/BlockSender.java:292-328)
    const int fr = fetch_recipe(ctx, (uint32_t)block_id, rec);
    if (fr < 0) return fr;
    if (!fr) return set_err(ctx, HDRF_E_NOTFOUND, "no recipe for this block (keep_recipes?)");
    const int64_t size = ((int64_t)rec[0] << 24) | (rec[1] << 16) | (rec[2] << 8) | rec[3];
    if (!out || cap < size) return set_err(ctx, HDRF_E_CAPACITY, "needs " + std::to_string(size) + " bytes");
    if (int rc = grow(ctx, &ctx->d_stage, &ctx->stage_cap, (uint64_t)size + 4096)) return rc;
    const int64_t got = reconstruct_body(ctx, rec.data(), (int64_t)rec.size(), ctx->d_stage, size, bad_chunk);
    if (got == HDRF_E_CORRUPT) {                         // the block's bytes are in the output anyway
        const std::string why = ctx->err;
        if (size) HIPCK(hipMemcpy(out, ctx->d_stage, size, hipMemcpyDeviceToHost));
        return set_err(ctx, HDRF_E_CORRUPT, "block " + std::to_string(block_id) + ", " + why);
    }
    if (got < 0) return got;
    if (got) HIPCK(hipMemcpy(out, ctx->d_stage, got, hipMemcpyDeviceToHost));
    return got;
}

extern "C" int64_t hdrf_reconstruct_block(hdrf_ctx *ctx, uint64_t block_id, uint8_t *out, int64_t cap)
{
    HDRF_LOCK(ctx);
    if (!ctx) return HDRF_E_INVAL;
    return reconstruct_block_body(ctx, block_id, out, cap, nullptr);
}

extern "C" int64_t hdrf_reconstruct_block_verified(hdrf_ctx *ctx, uint64_t block_id, uint8_t *out, int64_t cap,
                                                   int64_t *bad_chunk)
{
    HDRF_LOCK(ctx);
    if (!ctx || !bad_chunk) return HDRF_E_INVAL;
    return reconstruct_block_body(ctx, block_id, out, cap, bad_chunk);
}

// ---- batched, ranged reads (readv.hip; the arithmetic is read_plan.hpp's) -----------------------
// T, the bytes of output one gather wave fills.  HDRF_READ_TILE (4096, 8192 or 16384; read at every
// call, changes no result) is the knob scripts/read_speed.py measures with.
static uint32_t read_tile()
{
    const int t = env_int("HDRF_READ_TILE", (int)kReadTile);
    return t == 4096 || t == 8192 || t == 16384 ? (uint32_t)t : kReadTile;
}

// hdrf_read_batch with the arguments checked, the lock held and the batches in flight completed.
// Everything is enqueued on ctx->st; the one host wait follows the status read-back.
//
// A request that names a stored recipe whose block has a seek table (hdrf_seek_build) is served from
// the table: sk_span + sk_lookup (seek.hip) fill only the rows of the chunks under its range, sized by
// seek_row_bound before the device knows the span.  The descriptors are uploaded with the table-less
// requests first (`order`), so rv_lookup + rv_scan run over a prefix of them exactly as without tables,
// the seek kernels over the rest, and one rv_gather over all.  bad_chunk != nullptr (n entries): the
// verified read: vf_items + vf_hash re-hash every chunk under every successful range behind the gather.
static int read_batch_body(hdrf_ctx *ctx, int32_t n, hdrf_read_req *req, int64_t *bad_chunk = nullptr)
{
    const bool verify = bad_chunk != nullptr;
    ctx->seek_last_rows = ctx->seek_last_reqs = 0;
    if (n == 0) return 0;
    const uint32_t T = read_tile();
    const int H = ctx->H;
    std::vector<ReadDesc> desc((size_t)n);
    std::vector<int64_t> pre((size_t)n, 0);              // what the host decides: < 0 fails the request
    std::vector<uint64_t> dig_off((size_t)n, 0);         // caller-supplied digests: offset in the scratch
    std::vector<uint64_t> nrows((size_t)n, 0), nlen((size_t)n, 0);
    std::vector<SeekReq> sreq((size_t)n, SeekReq{});     // end != 0: the request is served from a table
    uint64_t dig_bytes = 0;
    int nseek = 0;
    for (int i = 0; i < n; i++) {
        if (verify) bad_chunk[i] = -1;
        const hdrf_read_req &q = req[i];
        ReadDesc &d = desc[(size_t)i];
        d = ReadDesc{};
        const hdrf_ctx::SeekLoc *tbl = nullptr;
        uint64_t size = 0, cnt = 0, clen = 0;
        if (q.recipe) {
            if (q.recipe_len < 4 || (q.recipe_len - 4) % H) pre[i] = HDRF_E_INVAL;
            else {
                size = ((uint64_t)q.recipe[0] << 24) | (q.recipe[1] << 16) | (q.recipe[2] << 8) | q.recipe[3];
                cnt = (uint64_t)(q.recipe_len - 4) / H;
            }
        } else {
            auto it = ctx->recipes.find((uint32_t)q.block_id);
            if (it == ctx->recipes.end()) pre[i] = HDRF_E_NOTFOUND;
            else {
                size = (uint64_t)ctx->lengths[(uint32_t)q.block_id];
                cnt = it->second.n;
                d.dig = (uint64_t)(uintptr_t)(ctx->rchunks[it->second.chunk] + it->second.off);
                auto sk = ctx->seeks.find((uint32_t)q.block_id);
                if (sk != ctx->seeks.end() && sk->second.n == it->second.n) tbl = &sk->second;
            }
        }
        if (!pre[i] && !read_clip(size, q.offset, q.length, &clen)) pre[i] = HDRF_E_INVAL;
        if (!pre[i] && clen && !q.dev_out) pre[i] = HDRF_E_INVAL;
        if (!pre[i] && cnt == 0 && size != 0) pre[i] = HDRF_E_DEVICE;      // a recipe without digests
        if (!pre[i] && cnt >= (1ull << 31)) pre[i] = HDRF_E_INVAL;
        if (pre[i]) cnt = clen = 0;                      // no rows, no tiles: the kernels pass it by
        else {
            d.out = (uint64_t)(uintptr_t)q.dev_out;
            d.n = (uint32_t)cnt;
            d.size = (uint32_t)size;
            d.off = (uint32_t)q.offset;
            d.len = (uint32_t)clen;
            if (q.recipe && cnt) {
                dig_off[i] = dig_bytes;
                dig_bytes += cnt * H;                    // H is a multiple of 4: the words stay aligned
            }
            if (tbl) {                                   // the span's rows; sk_span writes how many it has
                SeekReq &s = sreq[(size_t)i];
                s.end = (uint64_t)(uintptr_t)(ctx->schunks[tbl->chunk] + tbl->off);
                s.n = tbl->n;
                cnt = seek_row_bound(tbl->n, clen, tbl->minlen);
                s.cap = (uint32_t)cnt;
                d.n = 0;
                nseek++;
            }
        }
        nrows[(size_t)i] = cnt;
        nlen[(size_t)i] = clen;
    }
    // the upload order: the requests without a table, then those with one, each kind in the caller's order
    std::vector<int> order;
    order.reserve((size_t)n);
    for (int pass = 0; pass < 2; pass++)
        for (int i = 0; i < n; i++)
            if ((sreq[(size_t)i].end != 0) == (pass == 1)) order.push_back(i);
    const int nold = n - nseek;
    ReadPrefix px;
    uint64_t rows_old = 0;
    for (int p = 0; p < n; p++) {
        ReadDesc &d = desc[(size_t)order[(size_t)p]];
        if (p == nold) rows_old = px.rows;
        if (!px.add((uint32_t)nrows[(size_t)order[(size_t)p]], d.out, nlen[(size_t)order[(size_t)p]], T, &d.row0, &d.tile0))
            return set_err(ctx, HDRF_E_CAPACITY, "read batch: too many chunks or tiles for one call");
    }
    if (nseek == 0) rows_old = px.rows;
    ctx->seek_last_rows = (int64_t)px.rows;
    ctx->seek_last_reqs = nseek;
    Readable rd;
    readable_list(ctx, rd);
    const uint32_t ncont = (uint32_t)rd.cid.size();
    const bool extra = nseek || verify;                  // SeekReq rows and readable bounds behind the digests
    const ReadLayout L = read_layout((uint32_t)n, ncont, extra ? seek_extra_upload(dig_bytes, (uint32_t)n, ncont) : dig_bytes,
                                     px.rows, (uint32_t)sizeof(RdChunk));
    const SeekLayout SL = seek_layout(L, dig_bytes, (uint32_t)n, px.rows, (uint32_t)sizeof(VfReadItem), verify);
    if (int rc = grow(ctx, &ctx->d_rd, &ctx->rd_cap, SL.total)) return rc == HDRF_E_HIP ? HDRF_E_NOMEM : rc;
    uint8_t *R = ctx->d_rd;
    std::vector<uint8_t> up(L.upload, 0);
    for (int i = 0; i < n; i++) {
        if (pre[i] || !req[i].recipe || !desc[i].n) continue;
        desc[i].dig = (uint64_t)(uintptr_t)(R + L.o_dig + dig_off[i]);
        std::memcpy(up.data() + L.o_dig + dig_off[i], req[i].recipe + 4, (size_t)desc[i].n * H);
    }
    for (int p = 0; p < n; p++) {
        std::memcpy(up.data() + L.o_desc + (size_t)p * sizeof(ReadDesc), &desc[(size_t)order[(size_t)p]], sizeof(ReadDesc));
        if (extra) std::memcpy(up.data() + SL.o_sreq + (size_t)p * sizeof(SeekReq), &sreq[(size_t)order[(size_t)p]], sizeof(SeekReq));
    }
    if (ncont) {
        std::memcpy(up.data() + L.o_cid, rd.cid.data(), (size_t)ncont * 4);
        std::memcpy(up.data() + L.o_base, rd.base.data(), (size_t)ncont * 8);
        if (extra) std::memcpy(up.data() + SL.o_alloc, rd.alloc.data(), (size_t)ncont * 8);
    }
    hipStream_t st = ctx->st;
    std::vector<int> status((size_t)n, 0);               // in upload order, as everything read back below
    std::vector<uint32_t> vbad((size_t)n, 0xffffffffu);
    VfCounters vc{};
    ReadDesc *d_desc = (ReadDesc *)(R + L.o_desc);
    SeekReq *d_sreq = (SeekReq *)(R + SL.o_sreq);
    const uint32_t *d_cid = (const uint32_t *)(R + L.o_cid);
    const uint64_t *d_base = (const uint64_t *)(R + L.o_base);
    RdChunk *d_rows = (RdChunk *)(R + L.o_rows);
    int *d_status = (int *)(R + L.o_status);
    HIPCK(hipMemcpyAsync(R, up.data(), up.size(), hipMemcpyHostToDevice, st));
    HIPCK(hipMemsetAsync(d_status, 0, (size_t)n * 4, st));
    if (nseek == 0) {
        HIPCK(launch_readv(ctx->cfg.hasher, d_desc, n, (uint32_t)px.rows, (uint32_t)px.tiles, T, ctx->d_tab, ctx->cfg.index_log2,
                           tag_mask(ctx), d_cid, d_base, (int)ncont, d_rows, d_status, st));
    } else {
        // lookup + scan over the table-less prefix, span + lookup over the rest, then one gather over all
        HIPCK(launch_readv(ctx->cfg.hasher, d_desc, nold, (uint32_t)rows_old, 0, T, ctx->d_tab, ctx->cfg.index_log2,
                           tag_mask(ctx), d_cid, d_base, (int)ncont, d_rows, d_status, st));
        HIPCK(launch_seek_lookup(ctx->cfg.hasher, d_desc + nold, d_sreq + nold, nseek, (uint32_t)rows_old,
                                 (uint32_t)(px.rows - rows_old), ctx->d_tab, ctx->cfg.index_log2, tag_mask(ctx), d_cid,
                                 (int)ncont, d_rows, d_status + nold, st));
        HIPCK(launch_readv(ctx->cfg.hasher, d_desc, n, 0, (uint32_t)px.tiles, T, ctx->d_tab, ctx->cfg.index_log2,
                           tag_mask(ctx), d_cid, d_base, (int)ncont, d_rows, d_status, st));
    }
    if (verify) {
        HIPCK(hipMemsetAsync(R + SL.o_bad, 0xff, (size_t)n * 4, st));
        HIPCK(hipMemsetAsync(R + SL.o_cnt, 0, sizeof vc, st));
        HIPCK(launch_vf_read_items(ctx->cfg.hasher, d_desc, d_sreq, n, (uint32_t)px.rows, d_rows, d_status, d_base,
                                   (const uint64_t *)(R + SL.o_alloc), (VfReadItem *)(R + SL.o_items),
                                   (uint32_t *)(R + SL.o_bad), (VfCounters *)(R + SL.o_cnt), st));
        if (px.rows)
            HIPCK(launch_vf_hash_range(ctx->cfg.hasher, (const VfReadItem *)(R + SL.o_items), (uint32_t *)(R + SL.o_bad),
                                       (VfCounters *)(R + SL.o_cnt), vf_workgroups(ctx), st));
        HIPCK(hipMemcpyAsync(vbad.data(), R + SL.o_bad, (size_t)n * 4, hipMemcpyDeviceToHost, st));
        HIPCK(hipMemcpyAsync(&vc, R + SL.o_cnt, sizeof vc, hipMemcpyDeviceToHost, st));
    }
    HIPCK(hipMemcpyAsync(status.data(), d_status, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    HIPCK(hipStreamSynchronize(st));
    if (verify && vc.checked != vc.n_items) return set_err(ctx, HDRF_E_DEVICE, "verified read: not every chunk was hashed");
    std::vector<int> place((size_t)n, 0);                // request -> its place in the upload order
    for (int p = 0; p < n; p++) place[(size_t)order[(size_t)p]] = p;
    int first = 0;
    for (int i = 0; i < n; i++) {
        const int p = place[(size_t)i];
        const bool seek = sreq[(size_t)i].end != 0;
        int64_t r = pre[i];
        std::string why = r == HDRF_E_NOTFOUND ? "no recipe for this block (keep_recipes?)"
                          : r == HDRF_E_DEVICE ? "recipe without digests" : "bad recipe, offset past the block's end or no output";
        if (!r && (status[p] & kReadNotFound)) {
            r = HDRF_E_NOTFOUND;
            why = "a recipe digest is not in the index, or a container of the range is not readable";
        } else if (!r && (status[p] & kReadDevice)) {
            r = HDRF_E_DEVICE;
            why = seek ? "the block's seek table and the index disagree on a chunk's length (hdrf_seek_build again)"
                       : "chunk lengths do not add up to the recipe size";
        } else if (!r && verify && vbad[(size_t)p] != 0xffffffffu) {
            r = HDRF_E_CORRUPT;
            bad_chunk[i] = vbad[(size_t)p];
            if (!first) {                                // name the chunk: its digest, and the row the lookup made for it
                const uint32_t k = vbad[(size_t)p];
                std::vector<uint8_t> dg((size_t)H, 0);
                if (req[i].recipe) std::memcpy(dg.data(), req[i].recipe + 4 + (size_t)k * H, (size_t)H);
                else {
                    const hdrf_ctx::RecipeLoc &rl = ctx->recipes[(uint32_t)req[i].block_id];
                    HIPCK(hipMemcpy(dg.data(), ctx->rchunks[rl.chunk] + rl.off + (size_t)k * H, (size_t)H, hipMemcpyDeviceToHost));
                }
                SeekReq sq{};
                if (seek) HIPCK(hipMemcpy(&sq, d_sreq + p, sizeof sq, hipMemcpyDeviceToHost));
                RdChunk c{};
                HIPCK(hipMemcpy(&c, d_rows + desc[(size_t)i].row0 + (k - sq.k0), sizeof c, hipMemcpyDeviceToHost));
                const std::string where = c.slot < rd.cid.size() ? "container " + std::to_string(rd.cid[c.slot]) : std::string("no container");
                why = "recipe position " + std::to_string(k) + ": digest " + hex_digest(dg.data(), H) + ", " + where + " [" +
                      std::to_string(c.start) + ", " + std::to_string((uint64_t)c.start + c.len) +
                      "): the bytes hash to another digest (" + std::to_string(vc.n_bad) + " of " + std::to_string(vc.n_items) +
                      " chunks under the call's ranges)";
            }
        }
        req[i].result = r ? r : (int64_t)desc[i].len;     // (HDRF_E_CORRUPT: the bytes are in the output anyway)
        if (r && !first) first = set_err(ctx, (int)r, "read request " + std::to_string(i) + ": " + why);
    }
    return first;
}

static_assert(sizeof(hdrf_read_req) == 56, "hdrf_read_req: ctypes mirror ReadReq in hdrf_amd/lib.py");

// hdrf_read_batch (bad_chunk == nullptr) and hdrf_read_batch_verified
static int read_batch_entry(hdrf_ctx *ctx, int32_t n, hdrf_read_req *req, int64_t *bad_chunk)
{
    if (n < 0 || n > HDRF_READ_MAX_REQS) return set_err(ctx, HDRF_E_INVAL, "read batch: n outside [0, HDRF_READ_MAX_REQS]");
    if (ctx->G > 1) return set_err(ctx, HDRF_E_UNSUPPORTED, "ranged reads on node-global contexts");
    if (int rc = drain(ctx)) return rc;
    return read_batch_body(ctx, n, req, bad_chunk);
}

extern "C" int hdrf_read_batch(hdrf_ctx *ctx, int32_t n, hdrf_read_req *req)
{
    HDRF_LOCK(ctx);
    if (!ctx || !req) return HDRF_E_INVAL;
    return read_batch_entry(ctx, n, req, nullptr);
}

extern "C" int hdrf_read_batch_verified(hdrf_ctx *ctx, int32_t n, hdrf_read_req *req, int64_t *bad_chunk)
{
    HDRF_LOCK(ctx);
    if (!ctx || !req || !bad_chunk) return HDRF_E_INVAL;
    return read_batch_entry(ctx, n, req, bad_chunk);
}

// hdrf_read_range (bad_chunk == nullptr) and hdrf_read_range_verified
static int64_t read_range_body(hdrf_ctx *ctx, uint64_t block_id, uint64_t offset, uint64_t length, uint8_t *out, int64_t cap,
                               int64_t *bad_chunk)
{
    if (bad_chunk) *bad_chunk = -1;
    if (ctx->G > 1) return set_err(ctx, HDRF_E_UNSUPPORTED, "ranged reads on node-global contexts");
    if (int rc = drain(ctx)) return rc;                  // blocks in flight first: their recipes are SET
    uint64_t clen = 0;
    auto it = ctx->lengths.find((uint32_t)block_id);
    if (it != ctx->lengths.end() && ctx->recipes.count((uint32_t)block_id)) {
        if (!read_clip((uint64_t)it->second, offset, length, &clen))
            return set_err(ctx, HDRF_E_INVAL, "offset past the block's end");
        if (cap < (int64_t)clen || (clen && !out)) return set_err(ctx, HDRF_E_CAPACITY, "needs " + std::to_string(clen) + " bytes");
        if (int rc = grow(ctx, &ctx->d_stage, &ctx->stage_cap, clen + 4096)) return rc;
    }                                                    // (no recipe: the request reports it)
    hdrf_read_req q{};
    q.block_id = block_id;
    q.offset = offset;
    q.length = length;
    q.dev_out = ctx->d_stage;
    const int rc = read_batch_body(ctx, 1, &q, bad_chunk);
    if (rc == HDRF_E_CORRUPT && q.result == HDRF_E_CORRUPT) {        // the range's bytes are in the output anyway
        const std::string why = ctx->err;
        if (clen) HIPCK(hipMemcpy(out, ctx->d_stage, (size_t)clen, hipMemcpyDeviceToHost));
        return set_err(ctx, HDRF_E_CORRUPT, "block " + std::to_string(block_id) + ", " + why);
    }
    if (rc) return rc;
    if (q.result > 0) HIPCK(hipMemcpy(out, ctx->d_stage, (size_t)q.result, hipMemcpyDeviceToHost));
    return q.result;
}

extern "C" int64_t hdrf_read_range(hdrf_ctx *ctx, uint64_t block_id, uint64_t offset, uint64_t length, uint8_t *out,
                                   int64_t cap)
{
    HDRF_LOCK(ctx);
    if (!ctx) return HDRF_E_INVAL;
    return read_range_body(ctx, block_id, offset, length, out, cap, nullptr);
}

extern "C" int64_t hdrf_read_range_verified(hdrf_ctx *ctx, uint64_t block_id, uint64_t offset, uint64_t length, uint8_t *out,
                                            int64_t cap, int64_t *bad_chunk)
{
    HDRF_LOCK(ctx);
    if (!ctx || !bad_chunk) return HDRF_E_INVAL;
    return read_range_body(ctx, block_id, offset, length, out, cap, bad_chunk);
}
