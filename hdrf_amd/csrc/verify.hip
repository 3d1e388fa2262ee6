// verify.hip — fingerprint scrub and verified reads on gfx950: stored chunks re-hashed and compared
// with the digest that names them.
//
// The store is content-addressed: an index entry's key is the SHA-1 / SHA-224 of container[start,
// stop).  HDFS DataNodes run a block scanner and HDFS readers verify what they receive; here both
// are one hash kernel over bytes that already sit in HBM.
//
//   vf_collect — one lane per index-table slot of a slice: live entries of the wanted container(s)
//                are classified (container unreadable: skipped; range outside the container's
//                bytes: bad, reason 2; else an item) and appended wave-aggregated (ballot + mbcnt)
//                to an LDS batch that leaves with one global atomic
//   vf_hash    — persistent waves; a lane owns one item's whole compression chain (sha_core.hpp,
//                two blocks per iteration from one 132-B window) and, when it finishes, takes the
//                next item from the wave's register pool of 64 items reserved from a global
//                cursor, so a 1,000,000-B forced-cut chunk never leaves 63 lanes idle.  Scrub: items from
//                vf_collect, expected digest from the table entry (index_entry.hpp
//                entry_digest_words).  Verified read: the items are the RdChunk rows (rd_chunk.hpp) of
//                the lookup over the rebuilt block, expected digest from the recipe.  Verified ranged
//                read: the items are the VfReadItem rows of vf_items (seek.hip), each with a source of
//                its own.
//   vf_rows    — bad-list rows (table slot, reason) -> hdrf_bad_chunk records
#include <algorithm>

#define HDRF_SHA_K256_LINKAGE static
#include "sha_core.hpp"

namespace hdrf {

static_assert(sizeof(VfBadRow) == 44, "VfBadRow is hdrf_bad_chunk's layout");

struct VfItem {              // one chunk to hash
    uint32_t slot;           // table slot (scrub)
    uint32_t ridx;           // index in the readable-container list
    uint32_t start, len;
};
static_assert(sizeof(VfItem) == 16, "VfItem is one 16-B load");

// Persistent workgroups: workgroup x takes the 256-slot tiles x, x + gridDim.x, ... of the slice.
// Items are compacted into an LDS batch first (ballot + mbcnt per wave, an LDS counter per
// workgroup) and a batch leaves with ONE global atomic: with one global atomic per wave of 64
// slots (about nine items at the usual load) the appends serialised on the counter's line and the
// kernel ran at 180 GB/s of table, a third of the scrub's time.
constexpr uint32_t kVfBatch = 1024;          // LDS items; flushed above kVfBatch - 256
__global__ void __launch_bounds__(256) vf_collect_kernel(const IndexEntry *__restrict__ tab, uint64_t slot0,
                                                         uint32_t nslots, unsigned long long key, int64_t filter,
                                                         const uint32_t *__restrict__ cids,
                                                         const uint32_t *__restrict__ valid, int ncont,
                                                         VfItem *__restrict__ items, uint32_t *__restrict__ bad,
                                                         VfCounters *__restrict__ C)
{
    __shared__ VfItem s_items[kVfBatch];
    __shared__ uint32_t s_n, s_base, s_ent, s_skip;
    const uint32_t t = threadIdx.x;
    if (t == 0) { s_n = 0; s_ent = 0; s_skip = 0; }
    __syncthreads();
    auto flush = [&](uint32_t cnt) {                           // the whole workgroup, uniform
        if (t == 0) s_base = atomicAdd(&C->n_items, cnt);
        __syncthreads();
        for (uint32_t j = t; j < cnt; j += 256u) items[s_base + j] = s_items[j];
        __syncthreads();
        if (t == 0) s_n = 0;
        __syncthreads();
    };
    uint32_t n_ent = 0, n_skip = 0;
    for (uint32_t tile = blockIdx.x * 256u; tile < nslots; tile += gridDim.x * 256u) {   // uniform per workgroup
        const uint32_t i = tile + t;                           // every lane reaches the ballots below
        bool live = false;
        uint32_t cid = 0, start = 0, stop = 0;
        if (i < nslots) {
            const IndexEntry &e = tab[slot0 + i];
            live = tag_live(e.tag, key);
            cid = e.cid; start = e.start; stop = e.stop;
            if (filter >= 0 && (int64_t)cid != filter) live = false;
        }
        int kind = 0;                                          // 1 skipped, 2 bad range, 3 item
        uint32_t ridx = 0;
        if (live) {
            const int j = find_cid(cids, ncont, cid);
            if (j < 0) kind = 1;
            else if (start > stop || stop > valid[j]) kind = 2;
            else { kind = 3; ridx = (uint32_t)j; }
        }
        n_ent += live ? 1u : 0u;
        n_skip += kind == 1 ? 1u : 0u;
        const uint32_t bi = wave_append(&C->n_bad, kind == 2);  // (rare: straight to the global list)
        if (kind == 2) { bad[2 * (size_t)bi] = i; bad[2 * (size_t)bi + 1] = 2u; }
        const uint32_t ii = wave_append(&s_n, kind == 3);       // < kVfBatch: at most kVfBatch - 256 before the tile
        if (kind == 3) {
            VfItem it;
            it.slot = i; it.ridx = ridx; it.start = start; it.len = stop - start;
            s_items[ii] = it;
        }
        __syncthreads();
        const uint32_t cnt = s_n;
        __syncthreads();                                       // (the next tile's appends come after every read)
        if (cnt > kVfBatch - 256u) flush(cnt);
    }
    const uint32_t cnt = s_n;                                  // (the loop's last barrier is behind every append)
    if (cnt) flush(cnt);
    if (n_ent) atomicAdd(&s_ent, n_ent);
    if (n_skip) atomicAdd(&s_skip, n_skip);
    __syncthreads();
    if (t == 0) {
        if (s_ent) atomicAdd(&C->entries, s_ent);
        if (s_skip) atomicAdd(&C->skipped, s_skip);
    }
}

// MODE kVfScrub: items[0 .. *C.n_items) from vf_collect over slots slot0 + item.slot of tab;
// base / readable of an item = bases / allocs[item.ridx].
// MODE kVfBlock (verified read): item k = chunk k of the rebuilt block: chunks[k].len bytes at
// block_base + block_mis + chunks[k].off (block_base 4-B aligned, block_readable bytes readable from
// it), expected digest dig[k * HW ..]; the lowest failing k lands in C.first_bad_inv (as ~k).
// MODE kVfRange (verified ranged read): `items` holds *C.n_items VfReadItem rows from vf_items (seek.hip),
// each with its own source, readable bound and expected-digest address; the lowest failing recipe
// position of request r lands in bad[r].  The pool hands out item numbers, and a lane loads its item
// when it takes it.
constexpr int kVfScrub = 0, kVfBlock = 1, kVfRange = 2;
template <int HW, int MODE>
__global__ void __launch_bounds__(256) vf_hash_kernel(const VfItem *__restrict__ items, const RdChunk *__restrict__ chunks,
                                                      uint32_t n_read, const uint32_t *__restrict__ dig,
                                                      const IndexEntry *__restrict__ tab, uint64_t slot0,
                                                      const uint64_t *__restrict__ bases,
                                                      const uint64_t *__restrict__ allocs, const uint8_t *block_base,
                                                      uint32_t block_mis, uint64_t block_readable,
                                                      uint32_t *__restrict__ bad, VfCounters *__restrict__ C)
{
    constexpr bool READ = MODE == kVfBlock;
    const VfReadItem *ritems = (const VfReadItem *)items;     // (kVfRange)
    const uint32_t n = READ ? n_read : C->n_items;            // (written by vf_collect / vf_items, earlier on the stream)
    bool active = false, exhausted = false;
    uint32_t k = 0, s0 = 0, len = 0, T = 0, nb = 0, bi = 0;
    const uint8_t *base = block_base;
    uint64_t readable = block_readable;
    uint32_t st[8];
    set_iv<HW>(st);
    unsigned long long bytes = 0;
    uint32_t done_n = 0;
    const int l = lane_id();
    int head = 0, cntP = 0;                                    // the pool: items kbP .. kbP + cntP, one per lane
    uint32_t kbP = 0, p0 = 0, p1 = 0, p2 = 0, p3 = 0;          // slot (READ: k), readable index, start, len
    for (;;) {
        const bool done = active && bi == nb;                  // chain done: compare
        bool mism = false;
        if (done) {
            uint32_t want[HW];
            if (MODE == kVfRange) {
                const uint32_t *d = (const uint32_t *)(uintptr_t)ritems[k].dig;
#pragma unroll
                for (int i = 0; i < HW; i++) want[i] = d[i];
            } else if (READ) {
#pragma unroll
                for (int i = 0; i < HW; i++) want[i] = dig[(size_t)k * HW + i];
            } else {
                const IndexEntry &e = tab[slot0 + k];
                entry_digest_words<HW>(e.tag, e.ncopy, e.dig, want);
            }
#pragma unroll
            for (int i = 0; i < HW; i++) mism |= __builtin_bswap32(st[i]) != want[i];
            bytes += len;
            done_n++;
            active = false;
        }
        if (ballot64(mism)) {
            const uint32_t bi_ = wave_append(&C->n_bad, mism);
            if (mism) {
                if (MODE == kVfRange) atomicMin(bad + ritems[k].req, ritems[k].pos);
                else if (READ) atomicMax(&C->first_bad_inv, ~k);    // the lowest failing position
                else { bad[2 * (size_t)bi_] = k; bad[2 * (size_t)bi_ + 1] = 1u; }
            }
        }
        // The finished lanes take the next items from the wave's pool: 64 items reserved with one
        // atomic on the global cursor and kept in registers (one per lane), handed out with
        // ds_bpermutes as sha.hip hands out its chunk reservations.  (One atomic per iteration for
        // the lanes that finished in it was one per ~8 items of ~1 KB, all on one line.)
        for (;;) {
            const unsigned long long idle = ballot64(!active);
            if (!idle) break;
            if (head >= cntP) {
                if (exhausted) break;
                uint32_t got = 0;
                if (l == 0) got = atomicAdd(&C->cursor, 64u);
                kbP = rdfirst(got);
                cntP = kbP < n ? (int)min(64u, n - kbP) : 0;
                exhausted = (uint64_t)kbP + 64u >= n;          // wave-uniform
                head = 0;
                if (l < cntP) {
                    if (MODE == kVfRange) {
                        p0 = kbP + (uint32_t)l; p1 = 0u; p2 = 0u; p3 = 0u;
                    } else if (READ) {
                        const RdChunk c = chunks[kbP + l];
                        p0 = kbP + (uint32_t)l; p1 = 0u; p2 = c.off + block_mis; p3 = c.len;
                    } else {
                        const VfItem it = items[kbP + l];
                        p0 = it.slot; p1 = it.ridx; p2 = it.start; p3 = it.len;
                    }
                }
                if (cntP == 0) break;
            }
            const int rank = wave_rank(idle), avail = cntP - head, idx = min(head + rank, 63);
            const uint32_t q0 = (uint32_t)__shfl((int)p0, idx, 64), q1 = (uint32_t)__shfl((int)p1, idx, 64);
            const uint32_t q2 = (uint32_t)__shfl((int)p2, idx, 64), q3 = (uint32_t)__shfl((int)p3, idx, 64);
            if (!active && rank < avail) {
                k = q0;
                s0 = q2;
                len = q3;
                if (MODE == kVfRange) {
                    const VfReadItem it = ritems[q0];
                    base = (const uint8_t *)(uintptr_t)it.base;
                    readable = it.readable;
                    s0 = it.s0;
                    len = it.len;
                } else if (!READ) {
                    base = (const uint8_t *)(uintptr_t)bases[q1];
                    readable = allocs[q1];
                }
                T = len >> 6;
                nb = (len + 8) / 64 + 1;
                bi = 0;
                set_iv<HW>(st);
                active = true;
            }
            const int nidle = __popcll(idle);
            head += min(nidle, avail);
            if (nidle <= avail) break;
        }
        if (!ballot64(active)) break;
        if (active) sha_iter<HW>(base, readable, s0, len, T, nb, bi, st);   // sha_core.hpp
    }
    // hashed bytes and items: one atomic pair per wave
    bytes = wave_sum_u64(bytes);
    done_n = (uint32_t)wave_sum_u64(done_n);
    if (lane_id() == 0 && done_n) {
        atomicAdd(&C->bytes, bytes);
        atomicAdd(&C->checked, done_n);
    }
}

// bad-list rows [from, from + n) -> hdrf_bad_chunk-shaped records (VfBadRow)
template <int HW>
__global__ void __launch_bounds__(256) vf_rows_kernel(const uint32_t *__restrict__ bad, uint32_t from, uint32_t n,
                                                      const IndexEntry *__restrict__ tab, uint64_t slot0,
                                                      VfBadRow *__restrict__ out)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const IndexEntry &e = tab[slot0 + bad[2 * (size_t)(from + i)]];
    VfBadRow r;
    uint32_t dw[HW];
    entry_digest_words<HW>(e.tag, e.ncopy, e.dig, dw);
#pragma unroll
    for (int j = 0; j < 7; j++) r.dig[j] = j < HW ? dw[j] : 0u;
    r.cid = e.cid; r.start = e.start; r.stop = e.stop;
    r.why = (int32_t)bad[2 * (size_t)(from + i) + 1];
    out[i] = r;
}

hipError_t launch_vf_collect(const IndexEntry *tab, uint64_t slot0, uint32_t nslots, unsigned long long key,
                             int64_t filter, const uint32_t *cids, const uint32_t *valid, int ncont, void *items,
                             uint32_t *bad, VfCounters *C, int wgs, hipStream_t st)
{
    if (nslots == 0) return hipSuccess;
    hipLaunchKernelGGL(vf_collect_kernel, dim3(std::max(1u, std::min((uint32_t)wgs, (nslots + 255) / 256))), dim3(256), 0, st, tab, slot0, nslots, key, filter,
                       cids, valid, ncont, (VfItem *)items, bad, C);
    return hipGetLastError();
}

hipError_t launch_vf_hash_items(int hasher, const void *items, const IndexEntry *tab, uint64_t slot0,
                                const uint64_t *bases, const uint64_t *allocs, uint32_t *bad, VfCounters *C, int wgs,
                                hipStream_t st)
{
    const dim3 g(std::max(1, wgs));
    with_digest_words(hasher, [&](auto hw) {
        hipLaunchKernelGGL((vf_hash_kernel<decltype(hw)::value, kVfScrub>), g, dim3(256), 0, st, (const VfItem *)items, nullptr,
                           0u, nullptr, tab, slot0, bases, allocs, nullptr, 0u, 0ull, bad, C);
    });
    return hipGetLastError();
}

hipError_t launch_vf_hash_block(int hasher, const RdChunk *chunks, int n, const uint32_t *dig, const uint8_t *block,
                                uint64_t block_bytes, VfCounters *C, int wgs, hipStream_t st)
{
    if (n <= 0) return hipSuccess;
    // load_win fetches dwords at base + (pos & ~3): the base goes down to a dword, the rest into pos
    const uint32_t mis = (uint32_t)((uintptr_t)block & 3u);
    const dim3 g(std::max(1, std::min(wgs, (n + 255) / 256)));
    with_digest_words(hasher, [&](auto hw) {
        hipLaunchKernelGGL((vf_hash_kernel<decltype(hw)::value, kVfBlock>), g, dim3(256), 0, st, nullptr, chunks,
                           (uint32_t)n, dig, nullptr, 0ull, nullptr, nullptr, block - mis, mis, block_bytes + mis, nullptr, C);
    });
    return hipGetLastError();
}

hipError_t launch_vf_hash_range(int hasher, const VfReadItem *items, uint32_t *bad, VfCounters *C, int wgs, hipStream_t st)
{
    const dim3 g(std::max(1, wgs));
    with_digest_words(hasher, [&](auto hw) {
        hipLaunchKernelGGL((vf_hash_kernel<decltype(hw)::value, kVfRange>), g, dim3(256), 0, st, (const VfItem *)items, nullptr,
                           0u, nullptr, nullptr, 0ull, nullptr, nullptr, nullptr, 0u, 0ull, bad, C);
    });
    return hipGetLastError();
}

hipError_t launch_vf_rows(int hasher, const uint32_t *bad, uint32_t from, uint32_t n, const IndexEntry *tab,
                          uint64_t slot0, VfBadRow *out, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    const dim3 g((n + 255) / 256);
    with_digest_words(hasher, [&](auto hw) {
        hipLaunchKernelGGL(vf_rows_kernel<decltype(hw)::value>, g, dim3(256), 0, st, bad, from, n, tab, slot0, out);
    });
    return hipGetLastError();
}

}  // namespace hdrf
