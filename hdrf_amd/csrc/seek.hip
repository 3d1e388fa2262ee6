// seek.hip — seek tables on gfx950: a per-block table of chunk end offsets (seek_plan.hpp) with which a
// ranged read looks up only the chunks under its range, and the item list of the verified ranged read.
//
// Without a table a chunk's block offset is the sum of all earlier chunk lengths, and those live only in
// the index entries: rv_lookup + rv_scan (readv.hip) probe every digest of the recipe to serve 64 KiB.
//
//   sk_store  — hdrf_seek_build: one workgroup per recipe over the rows rv_lookup + rv_scan produced for
//               a zero-length request: end[k] = off + len into the seek store, and the smallest length
//               among chunks 0..n-2
//   sk_span   — one lane per request with a table: the two binary searches of seek_span over end[];
//               the span's row count, its first digest and its first chunk go where rv_gather (the
//               request's ReadDesc) and the kernels below (its SeekReq) read them
//   sk_lookup — one lane per row of the bounded row array; rows past a request's span exit.  The chunk's
//               RdChunk row from index_probe.hpp's probe_read_row, as rv_lookup; the block offset comes
//               from the table, not from a scan, and the entry's length must be the table's
//   vf_items  — verified ranged reads, after the gather: one lane per row of every request, with or
//               without a table.  A chunk that shares a byte with a successful request's range becomes
//               one VfReadItem of vf_hash (verify.hip): hashed from the output when it lies wholly
//               inside the range, from its container when the range cuts it
#include "index_probe.hpp"
#include "launchers.hpp"
#include "seek_plan.hpp"

namespace hdrf {

// grid nreq x 1024.  dst[r]: where the recipe's end[] goes; minlen[r]: 0xffffffff from the caller
__global__ void __launch_bounds__(1024) sk_store_kernel(const ReadDesc *__restrict__ req, const RdChunk *__restrict__ rows,
                                                        const int *__restrict__ status, const uint64_t *__restrict__ dst,
                                                        uint32_t *__restrict__ minlen)
{
    if (status[blockIdx.x]) return;                    // a failed id keeps no table
    const ReadDesc q = req[blockIdx.x];
    const RdChunk *c = rows + q.row0;
    uint32_t *end = (uint32_t *)(uintptr_t)dst[blockIdx.x];
    uint32_t m = 0xffffffffu;
    for (uint32_t k = threadIdx.x; k < q.n; k += 1024u) {
        const RdChunk ch = c[k];
        end[k] = ch.off + ch.len;
        if (k + 1 < q.n) m = min(m, ch.len);
    }
    m = ~wave_max_u32(~m);
    if (lane_id() == 0 && m != 0xffffffffu) atomicMin(minlen + blockIdx.x, m);
}

// grid ceil(nreq / 64) x 64 over the requests with a table.  A span the table cannot hold, or one
// longer than the rows set aside for it, fails the request (neither happens with a table hdrf_seek_build
// made for the recipe the request names).
template <int HW>
__global__ void __launch_bounds__(64) sk_span_kernel(ReadDesc *__restrict__ req, SeekReq *__restrict__ sq, uint32_t nreq,
                                                     int *__restrict__ status)
{
    const uint32_t r = blockIdx.x * 64u + threadIdx.x;
    if (r >= nreq) return;
    const ReadDesc q = req[r];
    if (q.len == 0) return;                            // no rows, no tiles: 0 bytes without a lookup
    const SeekReq s = sq[r];
    const uint32_t *end = (const uint32_t *)(uintptr_t)s.end;
    uint32_t k0 = 0, k1 = 0;
    uint32_t cnt = 0;
    if (seek_span(end, s.n, q.off, q.len, &k0, &k1)) cnt = k1 - k0 + 1;
    if (cnt == 0 || cnt > s.cap) {
        atomicOr(status + r, kReadDevice);
        cnt = 0;
    }
    req[r].n = cnt;
    req[r].dig = q.dig + (uint64_t)k0 * HW * 4;
    sq[r].k0 = k0;
}

// rows [row_base, row_base + nrows) belong to the requests req[0..nreq) (those with a table)
template <int HW>
__global__ void __launch_bounds__(256) sk_lookup_kernel(const ReadDesc *__restrict__ req, const SeekReq *__restrict__ sq,
                                                        uint32_t nreq, uint32_t row_base, uint32_t nrows,
                                                        const IndexEntry *__restrict__ tab, int log2cap,
                                                        unsigned long long tag_mask, const uint32_t *__restrict__ cids,
                                                        int ncont, RdChunk *__restrict__ rows, int *__restrict__ status)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= nrows) return;
    const uint32_t i = row_base + t;
    // requests without rows share their row0 with the next one: the last match is the row's owner
    const uint32_t r = last_le(nreq, i, [&](uint32_t m) { return req[m].row0; });
    const uint32_t j = i - req[r].row0;
    if (j >= req[r].n) return;                         // past the span (sk_span wrote n)
    const uint32_t k = sq[r].k0 + j;
    const uint32_t *end = (const uint32_t *)(uintptr_t)sq[r].end;
    const uint32_t *dig = (const uint32_t *)(uintptr_t)req[r].dig + (size_t)j * HW;
    uint32_t dw[HW];
#pragma unroll
    for (int w = 0; w < HW; w++) dw[w] = dig[w];
    RdChunk c;
    const bool found = probe_read_row<HW>(dw, tab, log2cap, tag_mask, cids, ncont, c);
    c.off = seek_start(end, k);
    if (!found) atomicOr(status + r, kReadNotFound);
    else if (c.len != end[k] - c.off) atomicOr(status + r, kReadDevice);      // the table and the index disagree
    else if (c.len != 0u && c.slot == kRdNoSlot) atomicOr(status + r, kReadNotFound);   // every span chunk with bytes is in the range
    rows[i] = c;
}

// one lane per row of all nreq requests (row0 ascends over them); sq[r].end == 0: a request without a table
template <int HW>
__global__ void __launch_bounds__(256) vf_items_kernel(const ReadDesc *__restrict__ req, const SeekReq *__restrict__ sq,
                                                       uint32_t nreq, uint32_t nrows, const RdChunk *__restrict__ rows,
                                                       const int *__restrict__ status, const uint64_t *__restrict__ bases,
                                                       const uint64_t *__restrict__ allocs, VfReadItem *__restrict__ items,
                                                       uint32_t *__restrict__ bad, VfCounters *__restrict__ C)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    bool want = false;
    VfReadItem it{};
    if (i < nrows) {
        const uint32_t r = last_le(nreq, i, [&](uint32_t m) { return req[m].row0; });
        const ReadDesc q = req[r];
        const uint32_t j = i - q.row0;
        if (j < q.n && !status[r]) {
            const RdChunk c = rows[i];
            const uint64_t r0 = q.off, r1 = (uint64_t)q.off + q.len, c1 = (uint64_t)c.off + c.len;
            want = c.len != 0u && c.off < r1 && c1 > r0;
            const bool inside = c.off >= r0 && c1 <= r1;
            const uint32_t pos = (sq[r].end ? sq[r].k0 : 0u) + j;
            if (want && !inside && (uint64_t)c.start + c.len > allocs[c.slot]) {
                want = false;                          // an entry past its container's bytes: nothing to hash
                atomicMin(bad + r, pos);
                atomicAdd(&C->n_bad, 1u);
            }
            if (want) {
                // (a chunk with bytes under a successful request's range has a readable container)
                const uint64_t a = inside ? q.out + (c.off - r0) : bases[c.slot] + c.start;
                const uint64_t lim = inside ? q.out + q.len : bases[c.slot] + allocs[c.slot];
                it.base = a & ~3ull;                   // load_win fetches dwords at base + (pos & ~3)
                it.readable = lim - it.base;
                it.dig = q.dig + (uint64_t)j * HW * 4;
                it.s0 = (uint32_t)(a & 3u);
                it.len = c.len;
                it.req = r;
                it.pos = pos;
            }
        }
    }
    const uint32_t at = wave_append(&C->n_items, want);
    if (want) items[at] = it;
}

hipError_t launch_seek_store(const ReadDesc *req, int nreq, const RdChunk *rows, const int *status, const uint64_t *dst,
                             uint32_t *minlen, hipStream_t st)
{
    if (nreq <= 0) return hipSuccess;
    hipLaunchKernelGGL(sk_store_kernel, dim3(nreq), dim3(1024), 0, st, req, rows, status, dst, minlen);
    return hipGetLastError();
}

hipError_t launch_seek_lookup(int hasher, ReadDesc *req, SeekReq *sq, int nreq, uint32_t row_base, uint32_t nrows,
                              const IndexEntry *tab, int log2cap, unsigned long long tag_mask, const uint32_t *cids,
                              int ncont, RdChunk *rows, int *status, hipStream_t st)
{
    if (nreq <= 0 || nrows == 0) return hipSuccess;    // (no rows: every request of them is empty)
    with_digest_words(hasher, [&](auto hw) {
        constexpr int HW = decltype(hw)::value;
        hipLaunchKernelGGL(sk_span_kernel<HW>, dim3((nreq + 63) / 64), dim3(64), 0, st, req, sq, (uint32_t)nreq, status);
        hipLaunchKernelGGL(sk_lookup_kernel<HW>, dim3((nrows + 255) / 256), dim3(256), 0, st, req, sq, (uint32_t)nreq,
                           row_base, nrows, tab, log2cap, tag_mask, cids, ncont, rows, status);
    });
    return hipGetLastError();
}

hipError_t launch_vf_read_items(int hasher, const ReadDesc *req, const SeekReq *sq, int nreq, uint32_t nrows,
                                const RdChunk *rows, const int *status, const uint64_t *bases, const uint64_t *allocs,
                                VfReadItem *items, uint32_t *bad, VfCounters *C, hipStream_t st)
{
    if (nreq <= 0 || nrows == 0) return hipSuccess;
    with_digest_words(hasher, [&](auto hw) {
        hipLaunchKernelGGL(vf_items_kernel<decltype(hw)::value>, dim3((nrows + 255) / 256), dim3(256), 0, st, req, sq,
                           (uint32_t)nreq, nrows, rows, status, bases, allocs, items, bad, C);
    });
    return hipGetLastError();
}

}  // namespace hdrf
