// seek_plan.hpp — the host arithmetic of the seek tables (hdrf_seek_build, api_seek.hip) and of the seek
// path of the batched, ranged read (api_views.hip read_batch_body; kernels in seek.hip).  No HIP in here:
// tests/cpp/seek_plan_test.cpp compiles it with g++ and checks it against per-byte models.
//
// The seek table of a recipe of n chunks is end[0..n), u32: end[k] is the block offset one past chunk k,
// so end[] ascends (not strictly: an empty chunk repeats its predecessor's value) and end[n - 1] is the
// block length.  With it the chunks under a byte range are found by two binary searches, and only
// their digests are looked up.
#pragma once
#include <stdint.h>

#include "read_plan.hpp"

namespace hdrf {

// One request beside its ReadDesc (uploaded with it; a request without a table has end == 0).
struct SeekReq {
    uint64_t end;        // device address of the table's end[] (4-B aligned)
    uint32_t n;          // chunks of the recipe
    uint32_t cap;        // rows the host set aside for the span (seek_row_bound)
    uint32_t k0;         // out (sk_span): recipe position of the span's first chunk
    uint32_t pad;
};
static_assert(sizeof(SeekReq) == 24, "SeekReq is read as three 8-B words");

// The span of a clipped range [off, off + clen), clen > 0, off + clen <= end[n - 1]: chunks k0..k1 with
//   k0 = the first k with end[k] > off            (the chunk holding byte off)
//   k1 = the first k with end[k] >= off + clen    (the chunk holding byte off + clen - 1)
// Both chunks have bytes, so empty chunks at either seam stay outside unless they lie between them.
// False when clen == 0 (no span) or the range does not lie inside the table (k1 would be n).
template <class E>
HDRF_PLAN_HD inline bool seek_span(E end, uint32_t n, uint64_t off, uint64_t clen, uint32_t *k0, uint32_t *k1)
{
    if (clen == 0 || n == 0) return false;
    uint32_t lo = 0, hi = n;                          // first k with end[k] > off
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if ((uint64_t)end[mid] > off) hi = mid; else lo = mid + 1;
    }
    *k0 = lo;
    hi = n;                                           // first k >= k0 with end[k] >= off + clen
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if ((uint64_t)end[mid] >= off + clen) hi = mid; else lo = mid + 1;
    }
    *k1 = lo;
    return lo < n;
}

// The block offset of chunk k's first byte.
template <class E>
HDRF_PLAN_HD inline uint32_t seek_start(E end, uint32_t k)
{
    return k ? end[k - 1] : 0u;
}

// Rows the host sets aside for a request's span before the device knows it.  The chunks strictly
// between the span's first and last lie wholly inside the range, and none of them is the recipe's last
// chunk, so each is at least minlen long (minlen: the smallest length among chunks 0..n-2): at most
// clen / minlen of them, plus the two edge chunks.  minlen == 0 bounds nothing: n rows.
inline uint64_t seek_row_bound(uint32_t n, uint64_t clen, uint32_t minlen)
{
    if (clen == 0) return 0;
    if (minlen == 0) return n;
    const uint64_t b = clen / minlen + 2;
    return b < n ? b : n;
}

// hdrf_seek_build works through its ids in groups: a group ends before the id that would take its
// rows past kSeekGroupRows (a single recipe may be longer: it is a group of its own) or its ids past
// max_ids.  Returns the end of the group that starts at `from`; cnt[i]: the chunks of id i's recipe.
constexpr uint64_t kSeekGroupRows = 4ull << 20;
inline int64_t seek_group_end(const uint32_t *cnt, int64_t n, int64_t from, int64_t max_ids)
{
    uint64_t rows = 0;
    int64_t i = from;
    for (; i < n && i - from < max_ids; i++) {
        if (i > from && rows + cnt[i] > kSeekGroupRows) break;
        rows += cnt[i];
    }
    return i;
}

// Where the seek path's and the verified read's pieces live in the read scratch, around read_plan.hpp's
// layout: the SeekReq rows and the containers' readable bounds travel in the one upload, behind the
// caller-supplied digests (they are counted into read_layout's dig_bytes); the verified read's
// per-request lowest bad position, its counters and its items follow the chunk rows (device only).
inline uint64_t seek_extra_upload(uint64_t dig_bytes, uint32_t nreq, uint32_t ncont)
{
    return read_up256(dig_bytes) + read_up256((uint64_t)nreq * sizeof(SeekReq)) + (uint64_t)ncont * 8;
}
struct SeekLayout {
    uint64_t o_sreq, o_alloc, o_bad, o_cnt, o_items, total;
};
inline SeekLayout seek_layout(const ReadLayout &L, uint64_t dig_bytes, uint32_t nreq, uint64_t rows, uint32_t item_bytes,
                              bool verify)
{
    SeekLayout S;
    S.o_sreq = L.o_dig + read_up256(dig_bytes);
    S.o_alloc = S.o_sreq + read_up256((uint64_t)nreq * sizeof(SeekReq));
    S.o_bad = L.total;
    S.o_cnt = read_up256(S.o_bad + (uint64_t)nreq * 4);
    S.o_items = S.o_cnt + 256;
    S.total = verify ? read_up256(S.o_items + rows * item_bytes) + 256 : L.total;
    return S;
}

}  // namespace hdrf
