// compact.hip — container compaction on gfx950 (hdrf_compact, api_compact.hip).
//
// The call names up to kCpMax closed containers (CpList, by value: the ids are searched in scalar
// registers).  What remains of each is the chunks that live index entries name, packed to the front
// in their old order.  No pass sorts: the order is kept by a cover map of one bit per container byte.
//   cp_collect — a streaming pass over the table, one lane per 64-B entry: table_walk.hpp's walk,
//                shared with gc_sweep.  A live entry of a listed container adds to the container's
//                counters (held in LDS, flushed once per workgroup) and becomes rows (compact_plan.hpp):
//                one per kCpPiece bytes.  It runs twice with the same grid: the first run only counts
//                the rows of each workgroup, so the second appends from a row base of its own
//                through an LDS counter (§13c: one returning global atomic on a single word held the
//                sweep at the rate of that word).  A range with stop <= start or stop > valid flags
//                the container and makes no row, so every later pass stays inside the container.
//   cp_cover   — one wave per row sets the row's bits: whole words are plain 16-B-wide vector stores
//                of ones, the two edge words atomicOr (neighbouring chunks share a word).
//   cp_scan    — eight workgroups per container: popcount and exclusive prefix over the map's words
//                (the scan step is common.hpp's wg1024_excl_scan, shared with rd_scan and rv_scan).
//                The popcount of a map differs from the sum of its ranges exactly when two overlap.
//   cp_moved   — one lane per row: the entries whose start changes, per container.
//   cp_gather  — one wave per row: old[a, b) -> image[new(a), ...), new(a) = prefix[a / 32] +
//                popc(word & low mask).  wave_copy<true> (bytes.hpp): 16-B nontemporal loads and stores
//                with a head and a tail, any alignment on both sides; the bytes are touched once.
//   cp_rewrite — one lane per row that carries a table slot: the entry's new start / stop, those
//                two words only.
#include <algorithm>

#include "bytes.hpp"
#include "compact_plan.hpp"
#include "launchers.hpp"
#include "table_walk.hpp"

namespace hdrf {

// new position of old byte p of a container whose map and prefix arrays are given (bit p is set)
__device__ __forceinline__ uint32_t cp_newpos(const uint32_t *__restrict__ map, const uint32_t *__restrict__ pre, uint32_t p)
{
    const uint32_t w = map[p >> 5];
    return pre[p >> 5] + (uint32_t)__popc(w & ((1u << (p & 31)) - 1u));
}

// Persistent workgroups: workgroup x takes the 256-slot tiles x, x + gridDim.x, ... of the table.
// kEmit = false: cc[] and wg[x] (the rows workgroup x will write); kEmit = true: the rows.
template <bool kEmit>
__global__ void __launch_bounds__(256) cp_collect_kernel(const IndexEntry *__restrict__ tab, uint64_t nslots,
                                                         unsigned long long key, const CpList list,
                                                         CpCount *__restrict__ cc, uint32_t *__restrict__ wg,
                                                         CpRow *__restrict__ rows, uint64_t row_cap,
                                                         uint32_t *__restrict__ err)
{
    __shared__ uint32_t s_row;                                 // the workgroup's next row
    __shared__ unsigned long long s_bytes[kCpMax];
    __shared__ uint32_t s_chunks[kCpMax], s_bad[kCpMax];
    const int t = (int)threadIdx.x, l = lane_id();
    if (t < kCpMax) { s_bytes[t] = 0; s_chunks[t] = 0; s_bad[t] = 0; }
    if (t == 0) s_row = 0;
    __syncthreads();
    if (kEmit) {
        const uint32_t before = wg_row_base(wg);
        if (l == 0 && before) atomicAdd(&s_row, before);
        __syncthreads();
    }
    table_walk(tab, nslots, [&](uint64_t slot, uint4 p0, uint4, uint4 p2, uint4) {
        const unsigned long long tag = (unsigned long long)p0.x | ((unsigned long long)p0.y << 32);
        const uint32_t cid = p2.x, start = p2.y, stop = p2.z;
        int j = -1;
        if (tag_live(tag, key)) {
#pragma unroll
            for (int k = 0; k < kCpMax; k++)
                if ((uint32_t)k < list.n && list.use[k] && list.id[k] == cid) j = k;
        }
        uint32_t np = 0;
        if (j >= 0) {
            const bool bad = stop <= start || stop > list.valid[j];
            if (!kEmit) {
                atomicAdd(&s_chunks[j], 1u);
                if (bad) atomicOr(&s_bad[j], 1u);
                else atomicAdd(&s_bytes[j], (unsigned long long)(stop - start));
            }
            if (!bad) np = cp_pieces(start, stop);
        }
        // one LDS atomic per wave: the wave's rows, lane by lane
        const uint32_t incl = wave_incl_scan(np);
        const uint32_t wtot = rdlane(incl, 63);
        if (wtot == 0) return;                                 // (uniform per wave)
        uint32_t base = 0;
        if (l == 0) base = atomicAdd(&s_row, wtot);
        base = rdfirst(base) + incl - np;
        if (kEmit) {
            for (uint32_t k = 0; k < np; k++) {
                const uint64_t row = (uint64_t)base + k;
                if (row >= row_cap) { atomicOr(err, 1u); break; }   // (never: the first run counted them)
                const uint32_t a = start + k * kCpPiece;
                const uint32_t b = stop - a > kCpPiece ? a + kCpPiece : stop;
                st16(rows + row, make_uint4(k ? kCpNoSlot : (uint32_t)slot, (uint32_t)j, a, b));
            }
        }
    });
    __syncthreads();
    if (!kEmit) {
        if (t == 0) wg[blockIdx.x] = s_row;
        if (t < kCpMax && s_chunks[t]) {                       // the workgroup's container counters leave LDS
            atomicAdd(&cc[t].chunks, (unsigned long long)s_chunks[t]);
            if (s_bytes[t]) atomicAdd(&cc[t].bytes, s_bytes[t]);
            if (s_bad[t]) atomicOr(&cc[t].bad, 1u);
        }
    }
}

// grid ceil(nrows / 4) x 256: wave w of the workgroup sets the bits [a, b) of row 4 * blockIdx.x + w
__global__ void __launch_bounds__(256) cp_cover_kernel(const CpRow *__restrict__ rows, uint32_t nrows,
                                                       uint32_t *__restrict__ maps, uint64_t map_words)
{
    const uint32_t i = blockIdx.x * 4u + (uint32_t)wave_id();
    if (i >= nrows) return;
    const uint4 rw = ld16(rows + i);
    const uint32_t a = rdfirst(rw.z), b = rdfirst(rw.w);
    uint32_t *map = maps + (uint64_t)rdfirst(rw.y) * map_words;
    const int l = lane_id();
    const uint32_t w0 = a >> 5, w1 = (b - 1) >> 5;             // first and last word touched (b > a)
    const uint32_t lo = ~0u << (a & 31), hi = ~0u >> (31 - ((b - 1) & 31));
    if (w0 == w1) {
        if (l == 0) atomicOr(map + w0, lo & hi);
        return;
    }
    if (l == 0) atomicOr(map + w0, lo);
    if (l == 1) atomicOr(map + w1, hi);
    for (uint32_t k = w0 + 1 + (uint32_t)l; k < w1; k += 64) map[k] = ~0u;   // (coalesced: 256 B per wave store)
}

// grid (kCpScanParts, n) x 1024: pre[k] = set bits of map[0..k) for the words of container blockIdx.y
// that hold its `valid` bytes; the total is added to cc[].covered.  Four words per thread and step.
// One workgroup walking a 32 MiB container's 2^20 words takes 256 dependent steps, and a call has at
// most 16 containers for 256 CUs: the words are cut into kCpScanParts parts of whole steps, and the
// workgroup of a part first sums the popcounts of the words before it (a streaming read with no
// step-to-step dependency, out of L2 for all but the first reader) instead of waiting for them.
constexpr int kCpScanParts = 8;
__global__ void __launch_bounds__(1024) cp_scan_kernel(const uint32_t *__restrict__ maps, uint32_t *__restrict__ pres,
                                                       uint64_t map_words, const CpList list, CpCount *__restrict__ cc)
{
    __shared__ uint32_t s_w[16];
    __shared__ unsigned long long s_carry;
    const int c = blockIdx.y, t = threadIdx.x;
    const uint32_t *map = maps + (uint64_t)c * map_words;
    uint32_t *pre = pres + (uint64_t)c * map_words;
    const uint32_t nw = list.use[c] ? (list.valid[c] + 31) / 32 : 0;   // <= map_words - 1
    const uint32_t per = ((nw + kCpScanParts - 1) / kCpScanParts + 4095) / 4096 * 4096;   // words of a part: whole steps
    const uint64_t lo64 = (uint64_t)blockIdx.x * per;
    if (lo64 >= nw) return;                                            // (uniform; an empty map has no part)
    const uint32_t w_lo = (uint32_t)lo64, w_hi = nw - w_lo > per ? w_lo + per : nw;
    if (t == 0) s_carry = 0;
    __syncthreads();
    unsigned long long before = 0;                                     // w_lo is a multiple of 4096: whole 16-B loads
    for (uint32_t k = 4u * (uint32_t)t; k < w_lo; k += 4096) {
        const uint4 m = ld16(map + k);
        before += __popc(m.x) + __popc(m.y) + __popc(m.z) + __popc(m.w);
    }
    before = wave_sum_u64(before);
    if (lane_id() == 0 && before) atomicAdd(&s_carry, before);
    __syncthreads();
    const unsigned long long first = s_carry;
    __syncthreads();
    for (uint32_t base = w_lo; base < w_hi; base += 4096) {            // uniform
        const uint32_t k = base + 4u * (uint32_t)t;
        uint4 m = make_uint4(0, 0, 0, 0);
        if (k + 4 <= nw) m = ld16(map + k);                            // (map strides are multiples of 256 B)
        else if (k < nw) {
            m.x = map[k];
            if (k + 1 < nw) m.y = map[k + 1];
            if (k + 2 < nw) m.z = map[k + 2];
        }
        const uint32_t c0 = __popc(m.x), c1 = __popc(m.y), c2 = __popc(m.z), c3 = __popc(m.w);
        const uint32_t v = c0 + c1 + c2 + c3;
        wg1024_excl_scan(v, s_w, &s_carry, [&](unsigned long long off) {
            const uint32_t e0 = (uint32_t)off;
            if (k + 4 <= nw) st16(pre + k, make_uint4(e0, e0 + c0, e0 + c0 + c1, e0 + c0 + c1 + c2));
            else if (k < nw) {
                pre[k] = e0;
                if (k + 1 < nw) pre[k + 1] = e0 + c0;
                if (k + 2 < nw) pre[k + 2] = e0 + c0 + c1;
            }
        });
    }
    if (t == 0 && s_carry != first) atomicAdd(&cc[c].covered, s_carry - first);    // (cleared by the caller)
}

// one lane per row: an entry (a row with a slot) whose start changes adds to its container's count
__global__ void __launch_bounds__(256) cp_moved_kernel(const CpRow *__restrict__ rows, uint32_t nrows,
                                                       const uint32_t *__restrict__ maps,
                                                       const uint32_t *__restrict__ pres, uint64_t map_words,
                                                       CpCount *__restrict__ cc)
{
    __shared__ uint32_t s_m[kCpMax];
    const int t = (int)threadIdx.x;
    if (t < kCpMax) s_m[t] = 0;
    __syncthreads();
    const uint32_t i = blockIdx.x * 256u + (uint32_t)t;
    if (i < nrows) {
        const uint4 rw = ld16(rows + i);
        if (rw.x != kCpNoSlot &&
            cp_newpos(maps + (uint64_t)rw.y * map_words, pres + (uint64_t)rw.y * map_words, rw.z) != rw.z)
            atomicAdd(&s_m[rw.y], 1u);
    }
    __syncthreads();
    if (t < kCpMax && s_m[t]) atomicAdd(&cc[t].moved, (unsigned long long)s_m[t]);
}

// grid ceil(nrows / 4) x 256: wave w of the workgroup copies row 4 * blockIdx.x + w, if the row's
// container is one of `go` (bit j: container j is compacted; the others' maps may be inconsistent)
__global__ void __launch_bounds__(256) cp_gather_kernel(const CpRow *__restrict__ rows, uint32_t nrows, uint32_t go,
                                                        const uint64_t *__restrict__ bases,
                                                        const uint32_t *__restrict__ maps,
                                                        const uint32_t *__restrict__ pres, uint64_t map_words,
                                                        uint8_t *__restrict__ img, uint64_t img_stride)
{
    const uint32_t i = blockIdx.x * 4u + (uint32_t)wave_id();
    if (i >= nrows) return;
    const uint4 rw = ld16(rows + i);
    const uint32_t j = rdfirst(rw.y), a = rdfirst(rw.z), b = rdfirst(rw.w);
    if (!((go >> j) & 1u)) return;
    const uint32_t na = cp_newpos(maps + (uint64_t)j * map_words, pres + (uint64_t)j * map_words, a);
    wave_copy<true>(img + (uint64_t)j * img_stride + na, (const uint8_t *)(uintptr_t)bases[j] + a, b - a);
}

// one lane per row with a slot, of the containers `go`: tab[slot].start / .stop <- the new range
__global__ void __launch_bounds__(256) cp_rewrite_kernel(const CpRow *__restrict__ rows, uint32_t nrows, uint32_t go,
                                                         const uint32_t *__restrict__ maps,
                                                         const uint32_t *__restrict__ pres, uint64_t map_words,
                                                         IndexEntry *__restrict__ tab)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= nrows) return;
    const uint4 rw = ld16(rows + i);
    if (rw.x == kCpNoSlot || !((go >> rw.y) & 1u)) return;
    IndexEntry *e = tab + rw.x;
    const uint32_t len = e->stop - e->start;                   // (the entry's own range: rw.w ends its first piece)
    const uint32_t ns = cp_newpos(maps + (uint64_t)rw.y * map_words, pres + (uint64_t)rw.y * map_words, rw.z);
    e->start = ns;
    e->stop = ns + len;
}

hipError_t launch_cp_collect(const IndexEntry *tab, int log2cap, unsigned long long key, const CpList &list, CpCount *cc,
                             uint32_t *wg, CpRow *rows, uint64_t row_cap, uint32_t *err, int wgs, hipStream_t st)
{
    if (log2cap < 8 || list.n > (uint32_t)kCpMax) return hipErrorInvalidValue;   // whole 256-slot tiles only
    const dim3 g(walk_grid(log2cap, wgs));
    if (!rows) hipLaunchKernelGGL(cp_collect_kernel<false>, g, dim3(256), 0, st, tab, 1ull << log2cap, key, list, cc, wg,
                                  rows, row_cap, err);
    else hipLaunchKernelGGL(cp_collect_kernel<true>, g, dim3(256), 0, st, tab, 1ull << log2cap, key, list, cc, wg, rows,
                            row_cap, err);
    return hipGetLastError();
}

hipError_t launch_cp_cover(const CpRow *rows, uint32_t nrows, const CpList &list, uint32_t *maps, uint32_t *pres,
                           uint64_t map_words, CpCount *cc, hipStream_t st)
{
    if (nrows) {
        hipLaunchKernelGGL(cp_cover_kernel, dim3((nrows + 3) / 4), dim3(256), 0, st, rows, nrows, maps, map_words);
    }
    hipLaunchKernelGGL(cp_scan_kernel, dim3(kCpScanParts, std::max(1u, list.n)), dim3(1024), 0, st, maps, pres, map_words,
                       list, cc);
    if (nrows)
        hipLaunchKernelGGL(cp_moved_kernel, dim3((nrows + 255) / 256), dim3(256), 0, st, rows, nrows, maps, pres, map_words,
                           cc);
    return hipGetLastError();
}

hipError_t launch_cp_gather(const CpRow *rows, uint32_t nrows, uint32_t go, const uint64_t *bases, const uint32_t *maps,
                            const uint32_t *pres, uint64_t map_words, uint8_t *img, uint64_t img_stride, hipStream_t st)
{
    if (!nrows || !go) return hipSuccess;
    hipLaunchKernelGGL(cp_gather_kernel, dim3((nrows + 3) / 4), dim3(256), 0, st, rows, nrows, go, bases, maps, pres,
                       map_words, img, img_stride);
    return hipGetLastError();
}

hipError_t launch_cp_rewrite(const CpRow *rows, uint32_t nrows, uint32_t go, const uint32_t *maps, const uint32_t *pres,
                             uint64_t map_words, IndexEntry *tab, hipStream_t st)
{
    if (!nrows || !go) return hipSuccess;
    hipLaunchKernelGGL(cp_rewrite_kernel, dim3((nrows + 255) / 256), dim3(256), 0, st, rows, nrows, go, maps, pres,
                       map_words, tab);
    return hipGetLastError();
}

}  // namespace hdrf
