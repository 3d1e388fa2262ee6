// gc.hip — index garbage collection on gfx950 (hdrf_gc, api_gc.hip).
//
// The live set is the set of digests of all recipes the context holds.  Two passes find it:
//   gc_mark   — one lane per recipe digest over all recipes laid end to end (gc_plan.hpp): probe_find,
//               then the entry's slot is set in a bitmap of one bit per table slot.  The same digest
//               occurs many times within and across recipes; a set bit is read before it is set again,
//               so only its first occurrences pay an atomic.
//   gc_sweep  — a streaming pass over the table, one lane per 64-B entry.  A wave reads its 64
//               entries as four fully coalesced 16-B loads per lane and turns them lane-major through
//               LDS.  Live and marked: appended to the survivor rows, in the layout idx_load_kernel
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
#include <algorithm>

#include "gc_plan.hpp"
#include "index_probe.hpp"
#include "launchers.hpp"

namespace hdrf {

// containers whose ids and counters a sweep workgroup keeps in LDS: 768 x 28 B beside the 16 KiB of
// entries is 37 KiB, so four workgroups share a CU's 160 KiB as the launch assumes (4 per CU)
constexpr int kGcLdsCont = 768;

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, d, 64);
        const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), d, 64);
        v += ((unsigned long long)hi << 32) | lo;
    }
    return v;
}

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
    __shared__ uint4 s_e[4][256];                              // per wave: its 64 entries, 4 KiB
    __shared__ uint32_t s_row, s_base;                         // the workgroup's next and first survivor row
    __shared__ unsigned long long s_kb[kGcLdsCont], s_db[kGcLdsCont];
    __shared__ uint32_t s_kc[kGcLdsCont], s_dc[kGcLdsCont];
    __shared__ uint32_t s_cid[kGcLdsCont];                     // the id list's first ids: the search stays in LDS
    const int t = (int)threadIdx.x, w = wave_id(), l = lane_id();
    const int nlds = min(ncont, kGcLdsCont);
    for (int j = t; j < nlds; j += 256) { s_kb[j] = 0; s_db[j] = 0; s_kc[j] = 0; s_dc[j] = 0; s_cid[j] = cids[j]; }
    if (t == 0) { s_row = 0; s_base = 0; }
    __syncthreads();
    if (dw_rows) {                                             // the rows of the workgroups before this one
        unsigned long long before = 0;
        for (uint32_t y = (uint32_t)t; y < blockIdx.x; y += 256u) before += wg[y];
        before = wave_sum_u64(before);
        if (l == 0 && before) { atomicAdd(&s_row, (uint32_t)before); atomicAdd(&s_base, (uint32_t)before); }
    }
    __syncthreads();
    unsigned long long n_ent = 0, n_kept = 0, n_drop = 0, b_kept = 0, b_drop = 0;
    const uint64_t tstride = (uint64_t)gridDim.x * 256u;
    // lane l's four 16-B pieces of the wave's 64 entries of a tile: piece k is bytes [(k * 64 + l) * 16, +16)
    auto fetch = [&](uint64_t tile, uint4 r[4]) {
        const uint8_t *wb = (const uint8_t *)(tab + tile + (uint64_t)w * 64);
#pragma unroll
        for (int k = 0; k < 4; k++) r[k] = ld16_nt(wb + (size_t)(k * 64 + l) * 16);
    };
    uint4 r[4] = {};
    if ((uint64_t)blockIdx.x * 256u < nslots) fetch((uint64_t)blockIdx.x * 256u, r);
    for (uint64_t tile = (uint64_t)blockIdx.x * 256u; tile < nslots; tile += tstride) {   // uniform
#pragma unroll
        for (int k = 0; k < 4; k++) s_e[w][k * 64 + l] = r[k];
        __syncthreads();
        const uint4 p0 = s_e[w][l * 4], p1 = s_e[w][l * 4 + 1], p2 = s_e[w][l * 4 + 2], p3 = s_e[w][l * 4 + 3];
        __syncthreads();                                       // (the next tile's stores come after every read)
        if (tile + tstride < nslots) fetch(tile + tstride, r); // in flight while this tile is classified
        const uint64_t slot = tile + (uint64_t)t;
        const unsigned long long tag = (unsigned long long)p0.x | ((unsigned long long)p0.y << 32);
        const bool live = tag_live(tag, key);
        n_ent += live ? 1u : 0u;
        if (!mark) continue;                                   // count only (uniform)
        const uint32_t ncopy = p1.w, cid = p2.x, start = p2.y, stop = p2.z;
        const bool kept = live && ((mark[slot >> 5] >> (slot & 31)) & 1u);
        const unsigned long long len = (unsigned long long)stop - start;   // (as the issue defines it: stop - start)
        bool unknown = false;
        if (live) {
            if (kept) { n_kept++; b_kept += len; } else { n_drop++; b_drop += len; }
            // the container id list, sorted: its first nlds ids from LDS (eight dependent global loads
            // per tile were most of the sweep's time), the rest, if the id lies there, from memory
            const bool far = nlds < ncont && cid > s_cid[nlds - 1];
            int lo = far ? nlds : 0, hi = far ? ncont : nlds;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if ((far ? cids[mid] : s_cid[mid]) < cid) lo = mid + 1; else hi = mid;
            }
            if (lo >= (far ? ncont : nlds) || (far ? cids[lo] : s_cid[lo]) != cid) {
                unknown = true;
                if (cid < (uint32_t)kGcCidBits) {
                    uint32_t *sw = seen + (cid >> 5);
                    const uint32_t bit = 1u << (cid & 31);
                    if (!(__hip_atomic_load(sw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit)) atomicOr(sw, bit);
                } else {
                    atomicOr(&C->err, 1u);
                }
            } else if (lo < kGcLdsCont) {
                if (kept) { atomicAdd(&s_kc[lo], 1u); atomicAdd(&s_kb[lo], len); }
                else { atomicAdd(&s_dc[lo], 1u); atomicAdd(&s_db[lo], len); }
            } else {
                if (kept) { atomicAdd(&cc[lo].kept_chunks, 1ull); atomicAdd(&cc[lo].kept_bytes, len); }
                else { atomicAdd(&cc[lo].dropped_chunks, 1ull); atomicAdd(&cc[lo].dropped_bytes, len); }
            }
        }
        const unsigned long long um = ballot64(unknown);
        if (um && l == (int)__builtin_ctzll(um)) atomicAdd(&C->n_unknown, (uint32_t)__popcll(um));
        if (!dw_rows) continue;                                // dry run: no survivor rows (uniform)
        const uint32_t row = wave_append(&s_row, kept);
        if (kept && row >= row_cap) atomicOr(&C->err, 2u);     // (never: a kept entry is a distinct live digest)
        if (kept && row < row_cap) {
            uint32_t dw[HW];                                  // the digest words the entry stands for (verify.hip vf_entry_words)
            if (HW == 5) {
                dw[0] = p3.z; dw[1] = p3.w;                    // dig[3..4]: digest bytes 0..7
            } else {
                const unsigned long long t56 = tag & kTag56;
                dw[0] = (uint32_t)t56;
                dw[1] = (uint32_t)(t56 >> 32) | (((ncopy >> 8) & 0xffu) << 24);
            }
            dw[2] = p2.w; dw[3] = p3.x; dw[4] = p3.y;          // dig[0..2]
            if (HW == 7) { dw[HW - 2] = p3.z; dw[HW - 1] = p3.w; }
#pragma unroll
            for (int k = 0; k < HW; k++) dw_rows[(size_t)row * HW + k] = dw[k];
            uint8_t *v = val_rows + (size_t)row * 11;          // chunkMeta.getMeta, DN/chunkMeta.java:62-77
            v[0] = (uint8_t)ncopy;
            v[1] = (uint8_t)(cid >> 16); v[2] = (uint8_t)(cid >> 8); v[3] = (uint8_t)cid;
            v[4] = (uint8_t)(start >> 16); v[5] = (uint8_t)(start >> 8); v[6] = (uint8_t)start;
            v[7] = (uint8_t)(stop >> 16); v[8] = (uint8_t)(stop >> 8); v[9] = (uint8_t)stop;
            v[10] = (uint8_t)(((start >> 20) & 0xF0) | ((stop >> 24) & 0x0F));
        }
    }
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
    const dim3 g((unsigned)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)std::min(std::max(1, wgs), (int)kGcSweepMaxWgs),
                                                                  nslots / 256)));
    if (dw_rows) hipLaunchKernelGGL(gc_count_kernel, g, dim3(256), 0, st, mark, nslots, wg, C);
    with_digest_words(hasher, [&](auto hw) {
        hipLaunchKernelGGL(gc_sweep_kernel<decltype(hw)::value>, g, dim3(256), 0, st, tab, nslots, key, mark, cids, ncont, cc,
                           seen, dw_rows, val_rows, row_cap, wg, C);
    });
    return hipGetLastError();
}

}  // namespace hdrf
