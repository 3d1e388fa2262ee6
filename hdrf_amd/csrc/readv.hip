// readv.hip — batched, ranged block reads (hdrf_read_batch) on gfx950: up to HDRF_READ_MAX_REQS byte
// ranges of blocks served by one set of launches, with no host wait between them.
//
// Reference: BlockSender serves [startOffset, startOffset + length) of a block by rebuilding the
// whole block and seeking into it (DN/BlockSender.java:612-619); here only the chunks that overlap
// the range are copied.  The requests of a call are described by ReadDesc rows (read_plan.hpp).
//
//   rv_lookup — one lane per (request, chunk) over all requests' digests: the chunk's RdChunk row
//               (rd_chunk.hpp) from index_probe.hpp's probe_read_row, the lookup body shared with
//               rd_lookup (read.hip).  An absent digest fails its request.
//   rv_scan   — one workgroup per request: block offsets of its chunks (common.hpp wg1024_excl_scan),
//               the total against the recipe size, and the readable-container check for the chunks
//               that overlap the request's range
//   rv_gather — partitioned by OUTPUT: one wave per tile of T output bytes (read_plan.hpp).  The
//               wave finds its request and the first chunk under its tile by binary search, then
//               copies the pieces of the consecutive chunks that fall in the tile.  A 2 MB chunk is
//               spread over 2 MB / T waves, and a 64 KiB range launches 64 KiB / T waves whatever
//               the block's size.
#include "bytes.hpp"
#include "index_probe.hpp"
#include "launchers.hpp"
#include "read_plan.hpp"

namespace hdrf {

template <int HW>
__global__ void __launch_bounds__(256) rv_lookup_kernel(const ReadDesc *__restrict__ req, uint32_t nreq, uint32_t nrows,
                                                        const IndexEntry *__restrict__ tab, int log2cap,
                                                        unsigned long long tag_mask, const uint32_t *__restrict__ cids,
                                                        int ncont, RdChunk *__restrict__ rows, int *__restrict__ status)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= nrows) return;
    // requests without rows share their row0 with the next one: the last match is the row's owner
    const uint32_t r = last_le(nreq, i, [&](uint32_t m) { return req[m].row0; });
    const uint32_t *dig = (const uint32_t *)(uintptr_t)req[r].dig + (size_t)(i - req[r].row0) * HW;
    uint32_t dw[HW];
#pragma unroll
    for (int k = 0; k < HW; k++) dw[k] = dig[k];
    RdChunk c;
    if (!probe_read_row<HW>(dw, tab, log2cap, tag_mask, cids, ncont, c))
        atomicOr(status + r, kReadNotFound);           // no offsets without its length
    rows[i] = c;
}

// grid nreq x 1024: off[k] = sum of len[0..k) over the request's rows; the total must be the recipe
// size; a chunk with bytes, no readable container and an overlap with the range fails the request
__global__ void __launch_bounds__(1024) rv_scan_kernel(const ReadDesc *__restrict__ req, RdChunk *__restrict__ rows,
                                                       int *__restrict__ status)
{
    __shared__ uint32_t s_w[16];
    __shared__ unsigned long long s_carry;
    const ReadDesc q = req[blockIdx.x];
    RdChunk *c = rows + q.row0;
    const int n = (int)q.n;
    const int t = threadIdx.x;
    const uint64_t r0 = q.off, r1 = (uint64_t)q.off + q.len;
    bool miss = false;
    if (t == 0) s_carry = 0;
    __syncthreads();
    for (int base = 0; base < n; base += 1024) {
        const int k = base + t;
        const uint32_t v = k < n ? c[k].len : 0u;
        wg1024_excl_scan(v, s_w, &s_carry, [&](uint64_t off) {
            if (k < n) {
                c[k].off = (uint32_t)off;
                miss |= v != 0u && c[k].slot == kRdNoSlot && off < r1 && off + v > r0;
            }
        });
    }
    if (miss) atomicOr(status + blockIdx.x, kReadNotFound);
    if (t == 0 && s_carry != q.size) atomicOr(status + blockIdx.x, kReadDevice);
}

// grid ceil(ntiles / 4) x 256: wave w of the workgroup fills output tile 4 * blockIdx.x + w
__global__ void __launch_bounds__(256) rv_gather_kernel(const ReadDesc *__restrict__ req, uint32_t nreq,
                                                        const int *__restrict__ status,
                                                        const RdChunk *__restrict__ rows,
                                                        const uint64_t *__restrict__ bases, uint32_t ntiles, uint32_t T)
{
    const uint32_t tile = blockIdx.x * 4u + (uint32_t)wave_id();
    if (tile >= ntiles) return;
    // requests without tiles share their tile0 with the next one: the last match owns the tile
    const uint32_t r = rdfirst(last_le(nreq, tile, [&](uint32_t m) { return req[m].tile0; }));
    if (status[r]) return;                             // a failed request writes nothing
    const ReadDesc q = req[r];
    uint64_t t0, t1;
    read_tile_span(q.out, q.len, T, tile - q.tile0, &t0, &t1);
    const RdChunk *c = rows + q.row0;
    uint64_t pos = q.off + t0;                         // block offsets [pos, end) land in this tile
    const uint64_t end = q.off + t1;
    // empty chunks share their offset with the next one: the last match holds the byte at pos
    uint32_t k = rdfirst(last_le(q.n, (uint32_t)pos, [&](uint32_t m) { return c[m].off; }));
    uint8_t *out = (uint8_t *)(uintptr_t)q.out;
    for (; pos < end && k < q.n; k++) {
        const RdChunk ch = c[k];
        const uint64_t cend = (uint64_t)ch.off + ch.len;
        if (cend <= pos) continue;
        const uint64_t pe = cend < end ? cend : end;
        if (ch.slot != kRdNoSlot)                      // (rv_scan failed the request otherwise)
            wave_copy(out + (pos - q.off), (const uint8_t *)(uintptr_t)bases[ch.slot] + ch.start + (pos - ch.off),
                      (uint32_t)(pe - pos));
        pos = pe;
    }
}

hipError_t launch_readv(int hasher, const ReadDesc *req, int nreq, uint32_t nrows, uint32_t ntiles, uint32_t T,
                        const IndexEntry *tab, int log2cap, unsigned long long tag_mask, const uint32_t *cids,
                        const uint64_t *bases, int ncont, RdChunk *c, int *status, hipStream_t st)
{
    if (nreq <= 0) return hipSuccess;
    if (nrows) {
        with_digest_words(hasher, [&](auto hw) {
            hipLaunchKernelGGL(rv_lookup_kernel<decltype(hw)::value>, dim3((nrows + 255) / 256), dim3(256), 0, st, req,
                               (uint32_t)nreq, nrows, tab, log2cap, tag_mask, cids, ncont, c, status);
        });
        hipLaunchKernelGGL(rv_scan_kernel, dim3(nreq), dim3(1024), 0, st, req, c, status);
    }
    if (ntiles)
        hipLaunchKernelGGL(rv_gather_kernel, dim3((ntiles + 3) / 4), dim3(256), 0, st, req, (uint32_t)nreq, status, c,
                           bases, ntiles, T);
    return hipGetLastError();
}

}  // namespace hdrf
