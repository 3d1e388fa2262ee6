// gc.hip — index garbage collection on gfx950 (hdrf_gc, api_gc.hip).
//
// The live set is the set of digests of all recipes the context holds.  Two passes find it:
//   gc_mark   — one lane per recipe digest over all recipes laid end to end (gc_plan.hpp): probe_find,
//               then the entry's slot is set in a bitmap of one bit per table slot.  The same digest
//               occurs many times within and across recipes; a set bit is read before it is set again,
//               so only its first occurrences pay an atomic.
//   gc_sweep  — a streaming pass over the table, one lane per 64-B entry: table_walk.hpp's walk (the
//               tile transposition through LDS, the prefetch and the row base of a workgroup are
//               there, shared with compact.hip's cp_collect); this file keeps what the sweep does with
//               an entry.  Live and marked: appended to the survivor rows, in the layout idx_load_kernel
//               reads, so the rebuild is the restore's kernel.  Live and unmarked: dropped.  Only a
//               live entry is ever marked, so the rows of a workgroup's tiles are counted from the
//               bitmap alone (gc_count) and each workgroup appends from a row base of its own
//               through an LDS counter, one LDS atomic per wave: with one returning global atomic per
//               wave on ONE counter the sweep ran at the rate of that word (3.25 ms for a table of
//               1 GiB that the pass otherwise reads in 0.41 ms).  Kept and dropped entries both add to
//               their container's counters, found by binary search in the sorted id list.  The
//               list's first kGcLdsCont ids and their counters live in LDS: the counters of a few
//               containers take every entry's add, and one global atomic per entry on so few
//               addresses would serialise at the memory side; and a search through memory is eight
//               dependent loads per tile, which was most of the sweep's time.
// Shared parts: the sorted-list search and wave_sum_u64 (common.hpp), an entry's digest words and its
// 11-byte value (index_entry.hpp).
#include "gc_plan.hpp"
#include "index_probe.hpp"
#include "launchers.hpp"
#include "table_walk.hpp"

namespace hdrf {

// containers whose ids and counters a sweep workgroup keeps in LDS: 768 x 28 B beside the 16 KiB of
// entries is 37 KiB, so four workgroups share a CU's 160 KiB as the launch assumes (4 per CU)
constexpr int kGcLdsCont = 768;

template <int HW>
__global__ void __launch_bounds__(256) gc_mark_kernel(const GcJob *__restrict__ jobs, uint32_t nj, uint64_t total,
                                                      const IndexEntry *__restrict__ tab, int log2cap,
                                                      unsigned long long key, uint32_t *__restrict__ mark,
                                                      GcCounters *__restrict__ C)
{
    unsigned long long miss = 0;
    const uint64_t stride = (uint64_t)gridDim.x * kGcTile;
    for (uint64_t i = (uint64_t)blockIdx.x * kGcTile + threadIdx.x; i < total; i += stride) {
        const GcJob jb = jobs[gc_find_job(jobs, nj, i)];
        const uint32_t *d = (const uint32_t *)(uintptr_t)jb.dig + (i - jb.first) * HW;
        uint32_t dw[HW];
#pragma unroll
        for (int k = 0; k < HW; k++) dw[k] = d[k];
        const IndexEntry *e = probe_find<HW>(dw, tab, log2cap, key);
        if (!e) { miss++; continue; }
        const uint64_t slot = (uint64_t)(e - tab);
        uint32_t *w = mark + (slot >> 5);
        const uint32_t bit = 1u << (slot & 31);
        if (!(__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit)) atomicOr(w, bit);
    }
    miss = wave_sum_u64(miss);                                 // (every lane is back here)
    if (lane_id() == 0 && miss) atomicAdd(&C->missing, miss);
}

// Marked slots of each sweep workgroup's tiles (launched with the sweep's grid): wg[x] for workgroup x.
__global__ void __launch_bounds__(256) gc_count_kernel(const uint32_t *__restrict__ mark, uint64_t nslots,
                                                       uint32_t *__restrict__ wg, GcCounters *__restrict__ C)
{
    __shared__ uint32_t s_n;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    unsigned long long n = 0;
    const uint64_t ntiles = nslots / 256;                      // 8 bitmap words per tile
    for (uint64_t tile = blockIdx.x + (uint64_t)threadIdx.x * gridDim.x; tile < ntiles; tile += 256ull * gridDim.x) {
        const uint4 a = ld16(mark + tile * 8), b = ld16(mark + tile * 8 + 4);
        n += __popc(a.x) + __popc(a.y) + __popc(a.z) + __popc(a.w) + __popc(b.x) + __popc(b.y) + __popc(b.z) + __popc(b.w);
    }
    n = wave_sum_u64(n);
    if (lane_id() == 0 && n) atomicAdd(&s_n, (uint32_t)n);
    __syncthreads();
    if (threadIdx.x == 0) {
        wg[blockIdx.x] = s_n;
        if (s_n) atomicAdd(&C->n_marked, s_n);
    }
}

// Persistent workgroups: workgroup x takes the 256-slot tiles x, x + gridDim.x, ... of the table
// (2^log2cap slots, a multiple of 256: index_log2 >= 10).  wg: gc_count's output for this grid.
template <int HW>
__global__ void __launch_bounds__(256) gc_sweep_kernel(const IndexEntry *__restrict__ tab, uint64_t nslots,
                                                       unsigned long long key, const uint32_t *__restrict__ mark,
                                                       const uint32_t *__restrict__ cids, int ncont,
                                                       GcContCount *__restrict__ cc, uint32_t *__restrict__ seen,
                                                       uint32_t *__restrict__ dw_rows, uint8_t *__restrict__ val_rows,
                                                       uint64_t row_cap, const uint32_t *__restrict__ wg,
                                                       GcCounters *__restrict__ C)
{
    __shared__ uint32_t s_row, s_base;                         // the workgroup's next and first survivor row
    __shared__ unsigned long long s_kb[kGcLdsCont], s_db[kGcLdsCont];
    __shared__ uint32_t s_kc[kGcLdsCont], s_dc[kGcLdsCont];
    __shared__ uint32_t s_cid[kGcLdsCont];                     // the id list's first ids: the search stays in LDS
    const int t = (int)threadIdx.x, l = lane_id();
    const int nlds = min(ncont, kGcLdsCont);
    for (int j = t; j < nlds; j += 256) { s_kb[j] = 0; s_db[j] = 0; s_kc[j] = 0; s_dc[j] = 0; s_cid[j] = cids[j]; }
    if (t == 0) { s_row = 0; s_base = 0; }
    __syncthreads();
    if (dw_rows) {
        const uint32_t before = wg_row_base(wg);
        if (l == 0 && before) { atomicAdd(&s_row, before); atomicAdd(&s_base, before); }
    }
    __syncthreads();
    unsigned long long n_ent = 0, n_kept = 0, n_drop = 0, b_kept = 0, b_drop = 0;
    table_walk(tab, nslots, [&](uint64_t slot, uint4 p0, uint4 p1, uint4 p2, uint4 p3) {
        const unsigned long long tag = (unsigned long long)p0.x | ((unsigned long long)p0.y << 32);
        const bool live = tag_live(tag, key);
        n_ent += live ? 1u : 0u;
        if (!mark) return;                                     // count only (uniform)
        const uint32_t ncopy = p1.w, cid = p2.x, start = p2.y, stop = p2.z;
        const bool kept = live && ((mark[slot >> 5] >> (slot & 31)) & 1u);
        const unsigned long long len = (unsigned long long)stop - start;   // (as the issue defines it: stop - start)
        bool unknown = false;
        if (live) {
            if (kept) { n_kept++; b_kept += len; } else { n_drop++; b_drop += len; }
            // the container id list, sorted: its first nlds ids from LDS (eight dependent global loads
            // per tile were most of the sweep's time), the rest, if the id lies there, from memory
            const bool far = nlds < ncont && cid > s_cid[nlds - 1];
            const int j = find_sorted(far ? nlds : 0, far ? ncont : nlds, cid,
                                      [&](int m) { return far ? cids[m] : s_cid[m]; });
            if (j < 0) {
                unknown = true;
                if (cid < (uint32_t)kGcCidBits) {
                    uint32_t *sw = seen + (cid >> 5);
                    const uint32_t bit = 1u << (cid & 31);
                    if (!(__hip_atomic_load(sw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit)) atomicOr(sw, bit);
                } else {
                    atomicOr(&C->err, 1u);
                }
            } else if (j < kGcLdsCont) {
                if (kept) { atomicAdd(&s_kc[j], 1u); atomicAdd(&s_kb[j], len); }
                else { atomicAdd(&s_dc[j], 1u); atomicAdd(&s_db[j], len); }
            } else {
                if (kept) { atomicAdd(&cc[j].kept_chunks, 1ull); atomicAdd(&cc[j].kept_bytes, len); }
                else { atomicAdd(&cc[j].dropped_chunks, 1ull); atomicAdd(&cc[j].dropped_bytes, len); }
            }
        }
        const unsigned long long um = ballot64(unknown);
        if (um && l == (int)__builtin_ctzll(um)) atomicAdd(&C->n_unknown, (uint32_t)__popcll(um));
        if (!dw_rows) return;                                  // dry run: no survivor rows (uniform)
        const uint32_t row = wave_append(&s_row, kept);
        if (kept && row >= row_cap) atomicOr(&C->err, 2u);     // (never: a kept entry is a distinct live digest)
        if (kept && row < row_cap) {
            const uint32_t dig[5] = {p2.w, p3.x, p3.y, p3.z, p3.w};
            uint32_t dw[HW];                                   // the digest words the entry stands for
            entry_digest_words<HW>(tag, ncopy, dig, dw);
#pragma unroll
            for (int k = 0; k < HW; k++) dw_rows[(size_t)row * HW + k] = dw[k];
            encode_value(ncopy, cid, start, stop, val_rows + (size_t)row * 11);
        }
    });
    __syncthreads();
    if (t == 0 && s_row != s_base) atomicAdd(&C->n_rows, s_row - s_base);
    for (int j = t; j < nlds; j += 256) {                      // the workgroup's container counters leave LDS
        if (s_kc[j]) { atomicAdd(&cc[j].kept_chunks, (unsigned long long)s_kc[j]); atomicAdd(&cc[j].kept_bytes, s_kb[j]); }
        if (s_dc[j]) { atomicAdd(&cc[j].dropped_chunks, (unsigned long long)s_dc[j]); atomicAdd(&cc[j].dropped_bytes, s_db[j]); }
    }
    n_ent = wave_sum_u64(n_ent);                               // entry totals: one atomic set per wave
    n_kept = wave_sum_u64(n_kept); n_drop = wave_sum_u64(n_drop);
    b_kept = wave_sum_u64(b_kept); b_drop = wave_sum_u64(b_drop);
    if (l == 0 && n_ent) {
        atomicAdd(&C->entries, n_ent);
        if (n_kept) { atomicAdd(&C->kept, n_kept); atomicAdd(&C->kept_bytes, b_kept); }
        if (n_drop) { atomicAdd(&C->dropped, n_drop); atomicAdd(&C->dropped_bytes, b_drop); }
    }
}

hipError_t launch_gc_mark(int hasher, const GcJob *jobs, uint32_t nj, uint64_t total, const IndexEntry *tab, int log2cap,
                          unsigned long long key, uint32_t *mark, GcCounters *C, hipStream_t st)
{
    if (total == 0 || nj == 0) return hipSuccess;
    const dim3 g(gc_grid(total));
    with_digest_words(hasher, [&](auto hw) {
        hipLaunchKernelGGL(gc_mark_kernel<decltype(hw)::value>, g, dim3(kGcTile), 0, st, jobs, nj, total, tab, log2cap, key,
                           mark, C);
    });
    return hipGetLastError();
}

hipError_t launch_gc_sweep(int hasher, const IndexEntry *tab, int log2cap, unsigned long long key, const uint32_t *mark,
                           const uint32_t *cids, int ncont, GcContCount *cc, uint32_t *seen, uint32_t *dw_rows,
                           uint8_t *val_rows, uint64_t row_cap, uint32_t *wg, GcCounters *C, int wgs, hipStream_t st)
{
    if (log2cap < 8 || ncont < 0) return hipErrorInvalidValue;   // whole 256-slot tiles only
    const uint64_t nslots = 1ull << log2cap;
    const dim3 g(walk_grid(log2cap, wgs));
    if (dw_rows) hipLaunchKernelGGL(gc_count_kernel, g, dim3(256), 0, st, mark, nslots, wg, C);
    with_digest_words(hasher, [&](auto hw) {
        hipLaunchKernelGGL(gc_sweep_kernel<decltype(hw)::value>, g, dim3(256), 0, st, tab, nslots, key, mark, cids, ncont, cc,
                           seen, dw_rows, val_rows, row_cap, wg, C);
    });
    return hipGetLastError();
}

}  // namespace hdrf
