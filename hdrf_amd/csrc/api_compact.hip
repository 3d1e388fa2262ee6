// api_compact.hip — libhdrf C-ABI: container compaction (kernels in compact.hip, the layout and
// eligibility arithmetic in compact_plan.hpp).
//
// hdrf_compact drains the pipeline and grows the read-side scratch (d_rd).  Unless HDRF_COMPACT_DRY it
// writes, for the rows it compacts only: the start / stop words of the index entries that name the
// container, the container's bytes (arena slot and compressed arena slot, or the loaded copy), its
// host record (ContainerInfo.len / .clen, Loaded.len; a loaded copy shadowed by a resident one is
// freed), and stats.closed_raw_bytes / closed_file_bytes — and `lost` when the commit fails.
#include "compact_plan.hpp"
#include "ctx.hpp"

static_assert(sizeof(hdrf_compact_row) == 56, "hdrf_compact_row: ctypes mirror CompactRow in hdrf_amd/lib.py");
static_assert(HDRF_COMPACT_MAX == kCpMax, "HDRF_COMPACT_MAX is compact_plan.hpp's kCpMax");

namespace {

// the call's staging: freed on every path
struct CpStaging {
    uint8_t *p = nullptr;
    ~CpStaging()
    {
        if (p) (void)hipFree(p);
    }
};

}  // namespace

extern "C" int64_t hdrf_compact(hdrf_ctx *ctx, int32_t flags, const uint32_t *ids, int32_t n, hdrf_compact_row *rows,
                                uint8_t *out, int64_t out_cap, int64_t *need)
{
    HDRF_LOCK(ctx);
    if (!ctx) return HDRF_E_INVAL;
    if (need) *need = 0;
    if (n < 0 || n > HDRF_COMPACT_MAX || (n && (!ids || !rows)) || (flags & ~HDRF_COMPACT_DRY) || out_cap < 0)
        return set_err(ctx, HDRF_E_INVAL, "hdrf_compact: bad arguments");
    for (int i = 0; i < n; i++)
        for (int k = 0; k < i; k++)
            if (ids[i] == ids[k]) return set_err(ctx, HDRF_E_INVAL, "hdrf_compact: container " + std::to_string(ids[i]) + " named twice");
    if (ctx->G > 1) return set_err(ctx, HDRF_E_UNSUPPORTED, "container compaction on node-global contexts");
    if (int rc = drain(ctx)) return rc;
    if (ctx->lost) return set_err(ctx, HDRF_E_HIP, "the context was lost by an earlier failure (hdrf_reset)");
    if (n == 0) return 0;
    const bool dry = (flags & HDRF_COMPACT_DRY) != 0;
    const hdrf_cfg &c = ctx->cfg;
    const bool lz = c.compressor == 2;
    const uint32_t cmax = c.container_max;
    const int log2cap = c.index_log2;
    hipStream_t st = ctx->st;

    // ---- phase A: nothing visible changes -------------------------------------------------------
    // eligibility from the host maps
    CpList list{};
    list.n = (uint32_t)n;
    int home[kCpMax] = {};
    uint64_t base[kCpMax] = {};
    for (int i = 0; i < n; i++) {
        hdrf_compact_row &r = rows[i];
        r = hdrf_compact_row{};
        r.id = ids[i];
        r.data_off = -1;
        auto ci = ctx->containers.find(ids[i]);
        auto lo = ctx->loaded.find(ids[i]);
        const bool resident = ci != ctx->containers.end();
        const bool pending = resident && c.retain_containers &&
                             std::find(ctx->pend_closed.begin(), ctx->pend_closed.end(), ids[i]) != ctx->pend_closed.end();
        home[i] = cp_classify(resident, resident && ci->second.closed, pending, lo != ctx->loaded.end());
        list.id[i] = ids[i];
        if (home[i] < 0) {
            r.status = home[i];
            continue;
        }
        list.use[i] = 1;
        if (home[i] == kCpArena) {
            list.valid[i] = ci->second.len;
            base[i] = (uint64_t)(uintptr_t)(ctx->d_arena + (size_t)ci->second.slot * cmax);
        } else {
            list.valid[i] = (uint32_t)lo->second.len;
            base[i] = (uint64_t)(uintptr_t)lo->second.ptr;
        }
        r.old_bytes = r.new_bytes = list.valid[i];
    }
    StageTimer tm("HDRF_COMPACT_TIMES", 10);             // collect / cover / gather / LZ4 / commit: scripts/compact_speed.py
    const uint32_t lz_segs = (uint32_t)((cmax + 261099) / 261100);       // launch_lz4's segments per container
    const int wgs = 4 * ctx->n_cu;
    // the first collect run: the containers' counters and the rows of each workgroup
    CpLayout L = cp_layout((uint32_t)n, cmax, 0, lz_segs);
    if (int rc = grow(ctx, &ctx->d_rd, &ctx->rd_cap, L.o_lz)) return rc == HDRF_E_HIP ? HDRF_E_NOMEM : rc;
    uint8_t *R = ctx->d_rd;
    CpCount cc[kCpMax] = {};
    std::vector<uint32_t> wg(kWalkMaxWgs, 0);
    HIPCK(hipMemsetAsync(R, 0, L.o_lz, st));
    tm.mark(0, st);
    HIPCK(launch_cp_collect(ctx->d_tab, log2cap, tag_mask(ctx), list, (CpCount *)(R + L.o_cnt), (uint32_t *)(R + L.o_wg),
                            nullptr, 0, nullptr, wgs, st));
    tm.mark(1, st);
    HIPCK(hipMemcpyAsync(cc, R + L.o_cnt, sizeof cc, hipMemcpyDeviceToHost, st));
    HIPCK(hipMemcpyAsync(wg.data(), R + L.o_wg, wg.size() * 4, hipMemcpyDeviceToHost, st));
    HIPCK(hipStreamSynchronize(st));
    uint64_t nrows = 0;
    for (uint32_t v : wg) nrows += v;
    if (nrows >= (1ull << 31)) return set_err(ctx, HDRF_E_CAPACITY, "hdrf_compact: too many chunk rows for one call");
    // the second run writes the rows; then the cover maps, their prefixes and the moved counts
    L = cp_layout((uint32_t)n, cmax, nrows, lz_segs);
    if (int rc = grow(ctx, &ctx->d_rd, &ctx->rd_cap, L.total)) return rc == HDRF_E_HIP ? HDRF_E_NOMEM : rc;
    R = ctx->d_rd;                                       // (it may have moved: everything is written again)
    const uint64_t map_words = L.map_stride / 4;
    CpRow *d_rows = (CpRow *)(R + L.o_rows);
    uint32_t *d_map = (uint32_t *)(R + L.o_map), *d_pre = (uint32_t *)(R + L.o_pre);
    uint32_t *d_err = (uint32_t *)(R + L.o_cnt + (uint64_t)kCpMax * sizeof(CpCount));
    CpCount up[kCpMax];
    std::memcpy(up, cc, sizeof up);
    HIPCK(hipMemsetAsync(R, 0, L.o_pre, st));            // counters, workgroup rows, the LZ4 block, the maps
    HIPCK(hipMemcpyAsync(R + L.o_cnt, up, sizeof up, hipMemcpyHostToDevice, st));
    HIPCK(hipMemcpyAsync(R + L.o_wg, wg.data(), wg.size() * 4, hipMemcpyHostToDevice, st));
    tm.mark(2, st);
    if (nrows)
        HIPCK(launch_cp_collect(ctx->d_tab, log2cap, tag_mask(ctx), list, (CpCount *)(R + L.o_cnt), (uint32_t *)(R + L.o_wg),
                                d_rows, nrows, d_err, wgs, st));
    tm.mark(3, st);
    HIPCK(launch_cp_cover(d_rows, (uint32_t)nrows, list, d_map, d_pre, map_words, (CpCount *)(R + L.o_cnt), st));
    tm.mark(4, st);
    uint32_t derr = 0;
    HIPCK(hipMemcpyAsync(cc, R + L.o_cnt, sizeof cc, hipMemcpyDeviceToHost, st));
    HIPCK(hipMemcpyAsync(&derr, d_err, 4, hipMemcpyDeviceToHost, st));
    HIPCK(hipStreamSynchronize(st));
    if (derr) return set_err(ctx, HDRF_E_DEVICE, "hdrf_compact: the second collect run found more rows than the first");
    uint32_t go = 0;
    int ngo = 0;
    int64_t raw_total = 0;
    for (int i = 0; i < n; i++) {
        if (home[i] < 0) continue;
        hdrf_compact_row &r = rows[i];
        r.status = cp_status(cc[i], list.valid[i]);
        r.chunks = (int64_t)cc[i].chunks;
        if (r.status == 2) r.new_bytes = 0;
        if (r.status != 0) continue;
        r.moved_chunks = (int64_t)cc[i].moved;
        r.new_bytes = (int64_t)cc[i].bytes;
        r.file_bytes = lz ? -1 : r.new_bytes;
        raw_total += r.new_bytes;
        go |= 1u << i;
        ngo++;
    }
    if (dry || !ngo) return ngo;
    if (!lz && out && raw_total > out_cap) {
        if (need) *need = raw_total;
        return set_err(ctx, HDRF_E_CAPACITY, "hdrf_compact: the files need " + std::to_string(raw_total) + " bytes");
    }
    // gather into the staging images, compress them into the staging slots
    const uint64_t lz_slot = lz ? lz4_slot_bytes(cmax) : 0;
    const CpStage SG = cp_stage((uint32_t)n, cmax, lz_slot);
    CpStaging stage;
    if (hipMalloc((void **)&stage.p, SG.total) != hipSuccess) {
        (void)hipGetLastError();
        stage.p = nullptr;
        return set_err(ctx, HDRF_E_NOMEM, "hdrf_compact: staging of " + std::to_string(SG.total) + " bytes");
    }
    uint8_t *img = stage.p + SG.o_img, *cimg = stage.p + SG.o_lz;
    uint64_t *d_base = (uint64_t *)(R + L.o_wg);         // (the workgroup rows are spent)
    HIPCK(hipMemcpyAsync(d_base, base, sizeof base, hipMemcpyHostToDevice, st));
    tm.mark(5, st);
    HIPCK(launch_cp_gather(d_rows, (uint32_t)nrows, go, d_base, d_map, d_pre, map_words, img, cmax, st));
    tm.mark(6, st);
    uint32_t flen[kCpMax] = {};
    int jof[kCpMax];                                     // container -> its ClosedRec
    if (lz) {
        ClosedRec rec[kCpMax] = {};
        uint32_t k = 0;
        for (int i = 0; i < n; i++) {
            jof[i] = -1;
            if (!((go >> i) & 1u)) continue;
            jof[i] = (int)k;
            rec[k++] = ClosedRec{ids[i], (uint32_t)i, (uint32_t)rows[i].new_bytes, 0};
        }
        uint8_t *Z = R + L.o_lz;
        HIPCK(hipMemcpyAsync(Z, rec, sizeof rec, hipMemcpyHostToDevice, st));
        HIPCK(hipMemcpyAsync(Z + kCpLzCount, &k, 4, hipMemcpyHostToDevice, st));
        HIPCK(launch_lz4((const ClosedRec *)Z, (const uint32_t *)(Z + kCpLzCount), kCpMax, cmax, img, cimg, lz_slot,
                         (uint32_t *)(Z + cp_lz_seglen()), (uint32_t *)(Z + kCpLzFileLen), (uint32_t *)(Z + kCpLzWork), st));
        HIPCK(hipMemcpyAsync(flen, Z + kCpLzFileLen, sizeof flen, hipMemcpyDeviceToHost, st));
    }
    tm.mark(7, st);
    HIPCK(hipStreamSynchronize(st));
    int64_t total = 0;
    for (int i = 0; i < n; i++) {
        if (!((go >> i) & 1u)) continue;
        if (lz) rows[i].file_bytes = (int64_t)flen[jof[i]];
        total += rows[i].file_bytes;
    }
    if (out && total > out_cap) {
        for (int i = 0; i < n; i++)
            if (((go >> i) & 1u) && lz) rows[i].file_bytes = -1;
        if (need) *need = total;
        return set_err(ctx, HDRF_E_CAPACITY, "hdrf_compact: the files need " + std::to_string(total) + " bytes");
    }
    if (out) {                                           // the caller's buffer is no state of the context
        int64_t used = 0;
        for (int i = 0; i < n; i++) {
            if (!((go >> i) & 1u)) continue;
            const uint8_t *src = lz ? cimg + (size_t)i * lz_slot : img + (size_t)i * cmax;
            if (rows[i].file_bytes)
                HIPCK(hipMemcpyAsync(out + used, src, (size_t)rows[i].file_bytes, hipMemcpyDeviceToHost, st));
            rows[i].data_off = used;
            used += rows[i].file_bytes;
        }
        HIPCK(hipStreamSynchronize(st));
    }

    // ---- phase B: commit ------------------------------------------------------------------------
    tm.mark(8, st);
    hipError_t e = hipSuccess;
    for (int i = 0; i < n && e == hipSuccess; i++) {
        if (!((go >> i) & 1u)) continue;
        e = hipMemcpyAsync((void *)(uintptr_t)base[i], img + (size_t)i * cmax, (size_t)rows[i].new_bytes,
                           hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess && lz && home[i] == kCpArena)
            e = hipMemcpyAsync(ctx->d_carena + (size_t)ctx->containers[ids[i]].slot * ctx->cslot, cimg + (size_t)i * lz_slot,
                               (size_t)rows[i].file_bytes, hipMemcpyDeviceToDevice, st);
    }
    if (e == hipSuccess) e = launch_cp_rewrite(d_rows, (uint32_t)nrows, go, d_map, d_pre, map_words, ctx->d_tab, st);
    tm.mark(9, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        ctx->lost = true;
        return set_err(ctx, HDRF_E_HIP, std::string("hdrf_compact commit: ") + hipGetErrorString(e) + " (hdrf_reset)");
    }
    for (int i = 0; i < n; i++) {
        if (!((go >> i) & 1u)) continue;
        const hdrf_compact_row &r = rows[i];
        if (home[i] == kCpArena) {
            ContainerInfo &ci = ctx->containers[ids[i]];
            const int64_t old_file = lz ? (int64_t)ci.clen : (int64_t)ci.len;
            ctx->stats.closed_raw_bytes -= r.old_bytes - r.new_bytes;
            ctx->stats.closed_file_bytes -= old_file - r.file_bytes;
            ci.len = (uint32_t)r.new_bytes;
            ci.clen = (uint32_t)r.file_bytes;
            auto lo = ctx->loaded.find(ids[i]);          // a loaded copy of the old file would be stale
            if (lo != ctx->loaded.end()) {
                (void)hipFree(lo->second.ptr);
                ctx->loaded.erase(lo);
            }
        } else {
            ctx->loaded[ids[i]].len = (uint64_t)r.new_bytes;
        }
    }
    if (tm.on) {
        long long moved_bytes = 0;
        for (int i = 0; i < n; i++)
            if ((go >> i) & 1u) moved_bytes += rows[i].new_bytes;
        fprintf(stderr, "hdrf_compact times: collect %.3f ms, cover %.3f ms, gather %.3f ms, lz4 %.3f ms, commit %.3f ms "
                        "(containers %d, rows %llu, gathered bytes %lld)\n",
                tm.ms(0, 1) + tm.ms(2, 3), tm.ms(3, 4), tm.ms(5, 6), lz ? tm.ms(6, 7) : 0.f, tm.ms(8, 9), ngo,
                (unsigned long long)nrows, moved_bytes);
    }
    return ngo;
}
