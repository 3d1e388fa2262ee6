// api_verify.hip — libhdrf C-ABI: the fingerprint scrub (the DataNode block scanner of a
// content-addressed store).  The verified reads share hdrf_reconstruct's body in api_views.hip.
//
// A view: drains the pipeline and writes nothing but the grown read-side scratch (d_rd).
#include "ctx.hpp"

static_assert(sizeof(hdrf_bad_chunk) == 44, "hdrf_bad_chunk: ctypes mirror BadChunk in hdrf_amd/lib.py");
static_assert(sizeof(hdrf_scrub_stats) == 40, "hdrf_scrub_stats: ctypes mirror ScrubStats in hdrf_amd/lib.py");
static_assert(sizeof(hdrf_bad_chunk) == sizeof(VfBadRow), "the device writes hdrf_bad_chunk records");

// The index table is walked in slices of 2^22 slots (collect, then hash), so the item and bad-list
// scratch is bounded whatever index_log2 is: 2^22 x (16 + 8) B = 96 MiB at most, less for a smaller
// table (scrub_slice_log2, ctx.hpp).
constexpr uint32_t kRowsPerCopy = 1u << 16;        // bad rows expanded and copied per round

extern "C" int64_t hdrf_scrub(hdrf_ctx *ctx, int64_t container, hdrf_bad_chunk *bad, int64_t cap, hdrf_scrub_stats *st_out)
{
    HDRF_LOCK(ctx);
    if (!ctx || cap < 0 || (cap && !bad) || container < -1 || container > 0xffffffffll) return HDRF_E_INVAL;
    if (ctx->G > 1) return set_err(ctx, HDRF_E_UNSUPPORTED, "scrub on node-global contexts");
    if (int rc = drain(ctx)) return rc;
    Readable rd;
    readable_list(ctx, rd);
    const int ncont = (int)rd.cid.size();
    if (container >= 0 && !std::binary_search(rd.cid.begin(), rd.cid.end(), (uint32_t)container))
        return set_err(ctx, HDRF_E_NOTFOUND, "container " + std::to_string(container) + " is neither resident nor loaded");
    const int slog = scrub_slice_log2(ctx);
    const uint64_t nslice = 1ull << slog, ntab = 1ull << ctx->cfg.index_log2;
    const uint64_t m = (uint64_t)std::max(1, ncont);
    const uint64_t o_cnt = 0;
    const uint64_t o_cid = 256, o_valid = (o_cid + m * 4 + 255) & ~255ull;
    const uint64_t o_base = (o_valid + m * 4 + 255) & ~255ull, o_alloc = (o_base + m * 8 + 255) & ~255ull;
    const uint64_t o_rows = (o_alloc + m * 8 + 255) & ~255ull;
    const uint64_t o_items = (o_rows + (uint64_t)kRowsPerCopy * sizeof(VfBadRow) + 255) & ~255ull;
    const uint64_t o_bad = (o_items + nslice * kVfItemBytes + 255) & ~255ull;
    const uint64_t o_end = o_bad + nslice * kVfBadBytes;
    if (int rc = grow(ctx, &ctx->d_rd, &ctx->rd_cap, o_end + 256)) return rc;
    uint8_t *R = ctx->d_rd;
    hipStream_t st = ctx->st;
    if (ncont) {
        HIPCK(hipMemcpyAsync(R + o_cid, rd.cid.data(), (size_t)ncont * 4, hipMemcpyHostToDevice, st));
        HIPCK(hipMemcpyAsync(R + o_valid, rd.valid.data(), (size_t)ncont * 4, hipMemcpyHostToDevice, st));
        HIPCK(hipMemcpyAsync(R + o_base, rd.base.data(), (size_t)ncont * 8, hipMemcpyHostToDevice, st));
        HIPCK(hipMemcpyAsync(R + o_alloc, rd.alloc.data(), (size_t)ncont * 8, hipMemcpyHostToDevice, st));
    }
    VfCounters *C = (VfCounters *)(R + o_cnt);
    uint32_t *d_bad = (uint32_t *)(R + o_bad);
    hdrf_scrub_stats S{};
    std::vector<hdrf_bad_chunk> rows;
    const int H = ctx->H;
    for (uint64_t s0 = 0; s0 < ntab; s0 += nslice) {
        HIPCK(hipMemsetAsync(C, 0, sizeof(VfCounters), st));
        HIPCK(launch_vf_collect(ctx->d_tab, s0, (uint32_t)nslice, tag_mask(ctx), container, (const uint32_t *)(R + o_cid),
                                (const uint32_t *)(R + o_valid), ncont, R + o_items, d_bad, C, 4 * vf_workgroups(ctx), st));
        HIPCK(launch_vf_hash_items(ctx->cfg.hasher, R + o_items, ctx->d_tab, s0, (const uint64_t *)(R + o_base),
                                   (const uint64_t *)(R + o_alloc), d_bad, C, vf_workgroups(ctx), st));
        VfCounters c{};
        HIPCK(hipMemcpyAsync(&c, C, sizeof c, hipMemcpyDeviceToHost, st));
        HIPCK(hipStreamSynchronize(st));
        if (c.checked != c.n_items || c.n_bad > nslice)
            return set_err(ctx, HDRF_E_DEVICE, "scrub: a slice's items were not all hashed");
        S.entries += c.entries;
        S.checked += c.checked;
        S.skipped += c.skipped;
        S.bytes += (int64_t)c.bytes;
        S.bad += c.n_bad;
        for (uint32_t from = 0; from < c.n_bad; from += kRowsPerCopy) {
            const uint32_t nr = std::min(kRowsPerCopy, c.n_bad - from);
            HIPCK(launch_vf_rows(ctx->cfg.hasher, d_bad, from, nr, ctx->d_tab, s0, (VfBadRow *)(R + o_rows), st));
            const size_t at = rows.size();
            rows.resize(at + nr);
            HIPCK(hipMemcpyAsync(rows.data() + at, R + o_rows, (size_t)nr * sizeof(VfBadRow), hipMemcpyDeviceToHost, st));
            HIPCK(hipStreamSynchronize(st));
        }
    }
    std::sort(rows.begin(), rows.end(), [H](const hdrf_bad_chunk &a, const hdrf_bad_chunk &b) {
        if (a.container != b.container) return a.container < b.container;
        if (a.start != b.start) return a.start < b.start;
        return std::memcmp(a.digest, b.digest, H) < 0;
    });
    const int64_t nout = std::min<int64_t>(cap, (int64_t)rows.size());
    if (nout) std::memcpy(bad, rows.data(), (size_t)nout * sizeof(hdrf_bad_chunk));
    if (st_out) *st_out = S;
    return S.bad;
}
