// The host arithmetic of the seek tables (hdrf_amd/csrc/seek_plan.hpp) against per-byte models
// (tests/test_seek.py compiles this with -fsanitize=address,undefined and runs it):
//   span     for every length list of a designed set and of an exhaustive cube (chunks of 0, 1, 2 and 5
//            bytes, up to 6 of them, so equal consecutive end values sit at both seams of some range),
//            every offset and every end (of a block above 64 B: those on a seam and one byte either side),
//            clipped as read_clip does: the span is
//            exactly the set of chunks that own a byte of the range, found by walking the range byte by
//            byte; off == size and ranges ending exactly on end[k] are among them; n = 0 and n = 1 too
//   bound    seek_row_bound covers the span of every one of those ranges, never exceeds n, is 0 for an
//            empty range and n when minlen is 0
//   groups   seek_group_end cuts any count list into consecutive groups that cover it, none above the
//            row or id limit unless it is a single id
//   layout   the extra regions are 256-B aligned, inside the upload resp. behind the rows, and disjoint
#include <algorithm>
#include <cstdio>
#include <vector>

#include "../../hdrf_amd/csrc/seek_plan.hpp"

using namespace hdrf;

#define CHECK(c)                                                  \
    do {                                                          \
        if (!(c)) {                                               \
            std::printf("FAIL line %d: %s\n", __LINE__, #c);      \
            return 1;                                             \
        }                                                         \
    } while (0)

// the chunk that owns block byte b, by walking the chunks
static int model_owner(const std::vector<uint32_t> &len, uint64_t b)
{
    uint64_t pos = 0;
    for (size_t k = 0; k < len.size(); k++) {
        if (b < pos + len[k]) return (int)k;
        pos += len[k];
    }
    return -1;
}

static int check_list(const std::vector<uint32_t> &len)
{
    const uint32_t n = (uint32_t)len.size();
    std::vector<uint32_t> endv(n);
    uint32_t *end = endv.data();                        // (null for n = 0: nothing may read it)
    uint64_t size = 0;
    uint32_t minlen = 0xffffffffu;                      // over chunks 0..n-2, as sk_store reduces it
    for (uint32_t k = 0; k < n; k++) {
        size += len[k];
        end[k] = (uint32_t)size;
        if (k + 1 < n) minlen = std::min(minlen, len[k]);
    }
    for (uint32_t k = 0; k < n; k++) CHECK(seek_start(end, k) == end[k] - len[k]);
    // every offset and length of a small block; of a larger one, those on a seam and one byte either side
    std::vector<uint64_t> pts;
    for (uint64_t v = 0; v <= size + 2; v++) {
        bool near = size <= 64 || v <= 1 || v + 1 >= size;
        for (uint32_t k = 0; k < n && !near; k++) near = v + 1 >= end[k] && v <= (uint64_t)end[k] + 1;
        if (near) pts.push_back(v);
    }
    for (uint64_t off : pts)
        for (uint64_t stop : pts) {
            if (off > size || (stop < off && stop != 0)) continue;
            const uint64_t length = stop < off ? 0 : stop - off;       // (the range ends on, before or behind a seam)
            uint64_t clen = 0;
            CHECK(read_clip(size, off, length, &clen));
            uint32_t k0 = 77, k1 = 77;
            const bool ok = seek_span(end, n, off, clen, &k0, &k1);
            const uint64_t bound = seek_row_bound(n, clen, minlen);
            CHECK(bound <= n);
            if (clen == 0) {                            // off == size, or length 0
                CHECK(!ok && bound == 0);
                continue;
            }
            CHECK(ok);
            int lo = -1, hi = -1;                       // the owners of the range's bytes, one at a time
            for (uint64_t b = off; b < off + clen; b++) {
                const int o = model_owner(len, b);
                CHECK(o >= 0);
                if (lo < 0) lo = o;
                CHECK(o >= hi);                         // owners ascend
                hi = o;
            }
            CHECK((int)k0 == lo && (int)k1 == hi);
            CHECK(len[k0] > 0 && len[k1] > 0);          // empty chunks at the seams stay outside
            CHECK(seek_start(end, k0) <= off && off < end[k0]);
            CHECK(end[k1] >= off + clen && seek_start(end, k1) < off + clen);
            CHECK((uint64_t)(k1 - k0 + 1) <= bound);
            if (minlen == 0) CHECK(bound == n);
            CHECK(seek_row_bound(n, clen, 0) == n);
        }
    uint32_t a = 0, b = 0;
    CHECK(!seek_span(end, n, 0, 0, &a, &b));
    CHECK(!seek_span(end, n, 0, size + 1, &a, &b));    // a range the table does not hold
    return 0;
}

static int test_span()
{
    const std::vector<std::vector<uint32_t>> designed = {
        {}, {0}, {1}, {7}, {1, 1, 702, 1, 5000, 1}, {0, 0, 1, 1, 0, 702, 0, 0, 1, 300, 1, 0, 0},
        {0, 5, 0}, {3, 0, 0, 3}, {0, 0, 0}, {64, 64, 64, 64}, {1000, 1, 1, 1, 1, 1000}, {2, 900, 2}};
    for (auto &l : designed)
        if (check_list(l)) return 1;
    const uint32_t alphabet[4] = {0, 1, 2, 5};
    for (uint32_t n = 0; n <= 6; n++) {
        uint32_t total = 1;
        for (uint32_t i = 0; i < n; i++) total *= 4;
        for (uint32_t code = 0; code < total; code++) {
            std::vector<uint32_t> l(n);
            uint32_t c = code;
            for (uint32_t i = 0; i < n; i++, c /= 4) l[i] = alphabet[c % 4];
            if (check_list(l)) return 1;
        }
    }
    // the bound's arithmetic at scale: a 64 KiB range over 906-B chunks, and the 64-bit edge
    CHECK(seek_row_bound(141000, 65536, 906) == 65536 / 906 + 2);
    CHECK(seek_row_bound(10, 65536, 906) == 10);
    CHECK(seek_row_bound(0xffffffffu, 0xffffffffull, 1) == 0xffffffffull);
    CHECK(seek_row_bound(5, 100, 0xffffffffu) == 2);   // a recipe of one chunk has no minlen
    return 0;
}

static int test_groups()
{
    const std::vector<std::vector<uint32_t>> lists = {
        {}, {0}, {5}, {(uint32_t)kSeekGroupRows}, {(uint32_t)kSeekGroupRows + 9, 1, 1},
        {1, (uint32_t)kSeekGroupRows, 1}, std::vector<uint32_t>(1000, 141000), std::vector<uint32_t>(700, 0),
        {3 << 20, 3 << 20, 1 << 20, 1 << 20, 2 << 20, 1}};
    for (auto &cnt : lists)
        for (int64_t max_ids : {1, 3, 256}) {
            const int64_t n = (int64_t)cnt.size();
            int64_t g0 = 0;
            while (g0 < n) {
                const int64_t g1 = seek_group_end(cnt.data(), n, g0, max_ids);
                CHECK(g1 > g0 && g1 <= n && g1 - g0 <= max_ids);
                uint64_t rows = 0;
                for (int64_t i = g0; i < g1; i++) rows += cnt[(size_t)i];
                CHECK(rows <= kSeekGroupRows || g1 - g0 == 1);
                if (g1 < n && g1 - g0 < max_ids) CHECK(rows + cnt[(size_t)g1] > kSeekGroupRows);   // groups are full
                g0 = g1;
            }
            CHECK(seek_group_end(cnt.data(), n, n, max_ids) == n);
        }
    return 0;
}

static int test_layout()
{
    for (uint32_t nreq : {1u, 3u, 256u})
        for (uint32_t ncont : {0u, 1u, 70u})
            for (uint64_t dig : {0ull, 20ull, 28ull * 141000})
                for (uint64_t rows : {0ull, 5ull, 1ull << 20})
                    for (bool verify : {false, true}) {
                        const ReadLayout L = read_layout(nreq, ncont, seek_extra_upload(dig, nreq, ncont), rows, 16);
                        const SeekLayout S = seek_layout(L, dig, nreq, rows, 40, verify);
                        CHECK(S.o_sreq % 256 == 0 && S.o_alloc % 256 == 0 && S.o_bad % 256 == 0 && S.o_cnt % 256 == 0 &&
                              S.o_items % 256 == 0);
                        CHECK(S.o_sreq >= L.o_dig + dig);
                        CHECK(S.o_alloc >= S.o_sreq + (uint64_t)nreq * sizeof(SeekReq));
                        CHECK(S.o_alloc + (uint64_t)ncont * 8 <= L.upload && L.upload <= L.o_status);
                        CHECK(S.o_bad >= L.o_rows + rows * 16);
                        CHECK(S.o_cnt >= S.o_bad + (uint64_t)nreq * 4 && S.o_items >= S.o_cnt + 256);
                        if (verify) CHECK(S.total >= S.o_items + rows * 40);
                        else CHECK(S.total == L.total);
                    }
    return 0;
}

int main()
{
    if (test_span() || test_groups() || test_layout()) return 1;
    std::printf("PASS\n");
    return 0;
}
